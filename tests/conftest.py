import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    from oracle import oracle as o
    o.lib()
    return o


@pytest.fixture(scope="session")
def nl():
    """The product package; GPU tests fail loudly if the HIP library or a device is missing."""
    import nightlight_amd
    from nightlight_amd import capi
    capi.load()
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need a real MI355X (there is no CPU fallback)")
    return nightlight_amd


@pytest.fixture(scope="session")
def experiments_lib(nl):
    """The experiments build (make -C nightlight_amd/csrc EXPERIMENTS=1, which build() runs: the four-pixels-per-wave
    replay, the split / persistent LDS-column pass, chunked passes, the guarded linear fit): the library the suite runs
    on when that is already this build, else nightlight_amd/libnlstack_exp.so opened beside it."""
    from nightlight_amd import capi
    lib = capi.load()
    if b"+experiments" not in lib.nl_version():
        lib = capi.open_library(capi.EXP_LIB_PATH)
        if b"+experiments" not in lib.nl_version():
            pytest.fail("%s is not the experiments build" % capi.EXP_LIB_PATH)
    return lib


@pytest.fixture
def experiments(experiments_lib, monkeypatch):
    """Runs the test on the experiments build: every handle the test creates goes through that library."""
    from nightlight_amd import capi
    monkeypatch.setattr(capi, "_lib", experiments_lib)
    return True
