import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (gfx950) GPU; parity tests through the C ABI")


@pytest.fixture(scope="session")
def oracle():
    from oracle import oracle as o
    o.build()
    return o


@pytest.fixture(scope="session")
def golden():
    import json
    d = os.path.join(ROOT, "tests", "golden")
    return {n[:-5]: json.load(open(os.path.join(d, n))) for n in os.listdir(d) if n.endswith(".json")}


@pytest.fixture(scope="session")
def efes_lib():
    from efes_amd import build
    build.build_lib()
    from efes_amd import _lib
    # Load through the binding before any test opens LIB_PATH itself: lib() imports torch first, so the
    # process keeps ONE HIP runtime (_lib._bind_process_hip_runtime) and the GPU tests that follow in
    # the same pytest process still find the device.
    _lib.lib()
    return _lib
