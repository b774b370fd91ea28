"""The prefilter's batch geometry block (FilterGeom / build_filter_geom, trew_amd/csrc/trew_common.hpp) is filled on the host and
only read on the device.  The library exports no entry point for it, so this test compiles the header's host function into a
small program of its own (tests/round_geometry_check.cpp) that compares the block, field by field, with get_segment and the
predicates evaluated directly: read lengths 20 .. 320, short, pair and segment mode, six (min_mer, max_mer) ranges, default flags,
TREW_FLAG_DEBUG_NO_JOINT and TREW_FLAG_DEBUG_NO_KLOOP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_agrees_with_the_geometry_evaluated_directly(tmp_path):
    cxx = shutil.which(os.environ.get("HOSTCXX", "g++"))
    if cxx is None:
        pytest.fail("no host C++ compiler (the build of the `trew` binary needs one as well)")
    exe = str(tmp_path / "round_geometry_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "trew_amd", "csrc"),
                    os.path.join(ROOT, "tests", "round_geometry_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    checks, mismatches = (int(x) for x in r.stdout.split()[0:3:2])
    assert mismatches == 0 and checks > 400_000, r.stdout
