"""The shapes and block lists the varblock tests share (tests/test_varblocks_cpu.py runs the cell-map builder over them,
tests/test_varblocks_gpu.py the kernel), and their seeded samples. Each case: (plane height, plane width, (cells_h, cells_w),
rows of (cy, cx, type)). The smallest shapes at which each piece of the kernel can go wrong."""
import numpy as np

F = np.float32

# 24 x 40 pixels = 3 x 5 cells: a 16x16 whose cell (1, 1) is interior (neither its block's top row nor its left column), a
# 16x8 and an 8x16 touching it, 8x8 blocks of five types
_MIX = [(0, 0, 4), (0, 2, 6), (0, 3, 7), (1, 3, 1), (1, 4, 2), (2, 0, 7), (2, 2, 3), (2, 3, 12), (2, 4, 13)]

# 512 x 512 pixels = 64 x 64 cells: all 27 types once, laid by hand; most of the lower right quarter belongs to no block
_ALL = [(0, 0, 24), (0, 32, 25), (32, 0, 26), (0, 48, 21), (16, 48, 22), (48, 0, 23), (16, 56, 18), (24, 56, 19), (48, 16, 20),
        (32, 32, 5), (32, 36, 8), (32, 37, 9), (36, 32, 10), (36, 34, 11), (40, 32, 4), (40, 34, 6), (40, 35, 7),
        (44, 32, 0), (44, 33, 1), (44, 34, 2), (44, 35, 3), (44, 36, 12), (44, 37, 13), (44, 38, 14), (44, 39, 15), (44, 40, 16),
        (44, 41, 17)]

CASES = {
    "a_8x8_one_dct8": (8, 8, (1, 1), [(0, 0, 0)]),
    "b_24x40_mix": (24, 40, (3, 5), _MIX),
    "c_21x37_ragged": (21, 37, (3, 5), _MIX),            # ragged row tail, rows 4-byte aligned only, blocks cut by the plane edge
    "d_512x512_all_types": (512, 512, (64, 64), _ALL),
    "e_32x32_upsampled": (32, 32, (2, 2), [(0, 0, 6), (0, 1, 0), (1, 1, 14)]),  # the block list of a 16 x 16 frame
    "f_13x10_under_dct16": (13, 10, (2, 2), [(0, 0, 4)]),
}


def samples(name, seed=11):
    """three float32 planes of the case: uniform in [-0.25, 1.5), and planted away from every block border: NaN, +-0, +-inf in
    each plane (at different pixels) and one pixel with R = G = B = -0.125, whose light is exactly 0 (a division by zero)"""
    h, w = CASES[name][:2]
    rng = np.random.default_rng(seed)
    planes = [rng.uniform(-0.25, 1.5, (h, w)).astype(F) for _ in range(3)]
    special = [F(np.nan), F(0.0), F(-0.0), F(np.inf), F(-np.inf)]
    for c in range(3):
        for k, v in enumerate(special):
            planes[c][2 + c, 1 + k] = v
    for c in range(3):
        planes[c][6, 3] = F(-0.125)
    return planes
