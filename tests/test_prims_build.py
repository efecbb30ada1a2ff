"""The primitives' test library (tests/prims_check.hip) builds for gfx950, loads
after the engine library and exports every entry point tests/test_prims_gpu.py
binds (no GPU call: this runs without one)."""
import os
import shutil
import subprocess

import pytest

import prims_lib

HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-C", os.path.join(prims_lib.ROOT, "jylis_amd"), "primcheck"], check=True)
    assert os.path.exists(prims_lib.LIB_PATH)
    return prims_lib.load()


def test_exports_every_bound_entry_point(lib):
    missing = [s for s in prims_lib.SIGNATURES if not hasattr(lib, s)]
    assert not missing, missing


def test_entry_points_stay_out_of_the_product_boundary():
    from jylis_amd import _lib
    assert not [s for s in _lib.SIGNATURES if s.startswith("jyt_")]
    header = open(os.path.join(prims_lib.ROOT, "include", "jylis_gpu.h")).read()
    assert "jyt_" not in header
