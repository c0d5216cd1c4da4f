#!/usr/bin/env python3
"""Record what JXLDecoder gives for every committed sample under every route (tests/golden/decode_routes.json): the whole
`stats` list and the CRC32 of every plane of every image decode() returns. Only the public surface is used, so the same
file records at any commit; tests/test_decode_routes_cpu.py and tests/test_decode_routes_gpu.py replay it through
`record()` and compare.

    python tests/golden/make_decode_routes.py oracle            # OracleBackend, default configuration: any machine
    python tests/golden/make_decode_routes.py device            # DeviceBackend, CONFIGS: needs the GPU

Each run rewrites its own section and leaves the other as it is. --commit names the commit the record is made at (default:
git's HEAD); --out writes the merged file somewhere else."""
import argparse
import glob
import json
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RECORD = os.path.join(HERE, "decode_routes.json")
SAMPLES = sorted(glob.glob(os.path.join(HERE, "samples", "*.jxl")))
NAMES = [os.path.splitext(os.path.basename(p))[0] for p in SAMPLES]
CONFIGS = {
    "default": {},
    "output": dict(device_output=True),
    "canvas": dict(device_canvas=True),
    "canvas+frames": dict(device_canvas=True, device_frames=True),
    "image": dict(device_image=True),
    "varblocks": dict(draw_varblocks=True, device_output=True),
    "all": dict(sparse_coeffs=True, device_splines=True, device_patches=True, device_output=True, device_canvas=True,
                device_palette=True, device_image=True, device_frames=True),
}
ORACLE_CONFIGS = {"default": {}}


def _plain(v):
    """JSON's view of a stats value: tuples are lists, numpy scalars Python's, keys strings"""
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.generic):
        return v.item()
    return v


def _crc(plane):
    a = bits = np.ascontiguousarray(plane)
    if a.dtype == np.float32:  # one NaN (Float.floatToIntBits): the payload of an invalid operation is the machine's
        bits = np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))
    return [a.dtype.str, list(a.shape), zlib.crc32(bits.tobytes())]


def record(path, backend, switches):
    """one sample decoded to the end under `switches`: dict(stats, images)"""
    from jxlatte_amd.decoder import JXLDecoder
    dec = JXLDecoder(path, backend=backend, **switches)
    images = []
    try:
        while True:
            im = dec.decode()
            if im is None:
                break
            images.append([_crc(p) for p in im.getBuffer(False)])
            im.close()
    finally:
        dec.close()
    return json.loads(json.dumps(dict(stats=_plain(dec.stats), images=images)))


def record_section(backend, configs):
    return {name: {cfg: record(path, backend, sw) for cfg, sw in configs.items()} for name, path in zip(NAMES, SAMPLES)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("section", choices=["oracle", "device"])
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=RECORD)
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    data = {}
    if os.path.exists(RECORD):
        with open(RECORD) as f:
            data = json.load(f)
    if a.section == "oracle":
        from oracle.pybackend import OracleBackend
        section = record_section(OracleBackend(), ORACLE_CONFIGS)
    else:
        from jxlatte_amd.decoder import DeviceBackend
        be = DeviceBackend()
        try:
            section = record_section(be, CONFIGS)
        finally:
            be.close()
    data[a.section] = dict(commit=commit, samples=section)
    with open(a.out, "w") as f:
        json.dump(data, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
