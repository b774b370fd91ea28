"""The CPU definitions of the four per-read motif measures (trew_amd/csrc/trew_measures_host.cpp) built on their own, with
AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program (tests/harness/measures_host_harness.cpp: no HIP,
no library): a clean run, and the same records as the library's trew_*_host return through trew_amd.capi.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from measure_cases import K32, make_reads
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("harness") / "measures_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "measures_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    return exe


def lines(records):
    return [" ".join(str(int(x)) for x in rec) for rec in records]


def expected_text(reads, motifs):
    """what the harness prints, from the library"""
    packed = capi.pack_reads(reads)
    out = ["annotate"] + lines(capi.annotate_host(packed, motifs).reshape(-1).tolist())
    out += ["tracts"] + lines(capi.tracts_host(packed, motifs, 3).reshape(-1).tolist())
    none, _, found0 = capi.intervals_host(packed, motifs, cap=0)
    assert len(none) == 0
    iv, counts, found = capi.intervals_host(packed, motifs)
    assert len(iv) == found
    out += ["intervals %d %d" % (found0, found)] + lines(iv.tolist()) + ["counts"] + lines(counts.reshape(-1, 2).tolist())
    v, hist, reads_with = capi.variants_host(packed, motifs)
    out += ["variants"] + lines(v.reshape(-1).tolist()) + ["histograms"]
    h, rw = hist.reshape(-1), reads_with.reshape(-1)
    out += ["%d %d %d" % (i, h[i], rw[i]) for i in np.flatnonzero((h != 0) | (rw != 0))]
    return "\n".join(out) + "\n"


@pytest.mark.parametrize("motifs", [["TTG"], ["TTAGGG"], [K32], ["TTAGGG", "TTG", K32]], ids=["k3", "k6", "k32", "k6_k3_k32"])
@pytest.mark.parametrize("which", ["reads", "no_reads"])
def test_definitions_run_clean_under_sanitizers_and_agree_with_the_library(harness, which, motifs):
    reads = make_reads() if which == "reads" else []
    r = subprocess.run([harness] + motifs, input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == b""
    assert r.stdout.decode() == expected_text(reads, motifs)
