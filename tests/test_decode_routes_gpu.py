"""GPU: every committed sample decoded to the end with DeviceBackend under every route configuration gives the recorded `stats`
list and the recorded CRC32 of every plane of every image (tests/golden/decode_routes.json, section "device", made on the
MI355X by tests/golden/make_decode_routes.py at the commit named in the file). A sample or configuration the record lacks
fails."""
import pytest

from jxlatte_amd import host
from jxlatte_amd.decoder import DeviceBackend
from test_decode_routes_cpu import M, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend(ctx):
    be = DeviceBackend.__new__(DeviceBackend)
    be.host, be.ctx, be.palette_log = host, ctx, []
    return be


@pytest.mark.parametrize("cfg", list(M.CONFIGS))
@pytest.mark.parametrize("name", M.NAMES)
def test_device_decode_equals_the_record(backend, name, cfg):
    check("device", backend, name, cfg, M.CONFIGS[cfg])
