"""CPU: every committed sample decoded to the end with OracleBackend gives the recorded `stats` list and the recorded CRC32 of
every plane of every image (tests/golden/decode_routes.json, section "oracle", made by tests/golden/make_decode_routes.py at
the commit named in the file). A sample or configuration the record lacks fails."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_decode_routes", os.path.join(ROOT, "tests", "golden", "make_decode_routes.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

with open(M.RECORD) as f:
    RECORD = json.load(f)


def check(section, backend, name, cfg, switches):
    """shared with tests/test_decode_routes_gpu.py"""
    want = RECORD.get(section, {}).get("samples", {}).get(name, {}).get(cfg)
    assert want is not None, "%s / %s is not in section %r of the record" % (name, cfg, section)
    got = M.record(M.SAMPLES[M.NAMES.index(name)], backend, switches)
    assert len(got["stats"]) == len(want["stats"]), (name, cfg)
    for k, (g, w) in enumerate(zip(got["stats"], want["stats"])):
        assert g == w, "%s / %s: stats[%d] differs: %r" % (name, cfg, k, {key: (g.get(key), w.get(key)) for key in set(g) | set(w)
                                                                          if g.get(key) != w.get(key)})
    assert got["images"] == want["images"], "%s / %s: planes differ (dtype, shape, CRC32 per plane)" % (name, cfg)


@pytest.fixture(scope="module")
def oracle():
    from oracle.pybackend import OracleBackend
    return OracleBackend()


@pytest.mark.parametrize("cfg", sorted(M.ORACLE_CONFIGS))
@pytest.mark.parametrize("name", M.NAMES)
def test_oracle_decode_equals_the_record(oracle, name, cfg):
    check("oracle", oracle, name, cfg, M.ORACLE_CONFIGS[cfg])
