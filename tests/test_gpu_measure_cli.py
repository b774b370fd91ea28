"""The file path all twelve per-read measures share (host/process.cpp: process_annotate, the serial chunk reader, the
workers' folds, add_totals and the sorts at the end) with many chunks a file: one generated FASTQ of a few hundred KB, cut
by TREW_MEASURE_CHUNK_BYTES into about a hundred (4096) or a few hundred (1777) batches that one, three or sixteen workers
share, must give byte for byte what the CPU definitions (capi.*_host) give over the whole file -- plain, gzip, BGZF, given
twice, with CRLF line ends -- and a read that does not fit a chunk must end the run cleanly.  Where the chunk borders
fall is taken from chunk_spans (tests/test_fastq_chunks_cpu.py, checked there against the product's reader)."""
import gzip
import os
import re
import subprocess

import pytest

import measure_cli_cases as M
from test_bgzf_cpu import write_bgzf
from test_fastq_chunks_cpu import chunk_reads, chunk_spans

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
CHUNKS = [M.CHUNK, 1777, None]
THREADS = ["2", "4", "17"]  # one, three and sixteen workers


class TheFile:
    def __init__(self, folder):
        self.data = M.make_file()
        self.reads = M.reads_of(self.data)
        self.host = M.host_results(self.reads)
        self.path = str(folder / "measures.fastq")
        with open(self.path, "wb") as f:
            f.write(self.data)
        self.want = {name: M.expected(name, [self.path], self.reads, self.host[name]) for name in M.COMMANDS}
        self.spans = chunk_spans(self.data, M.CHUNK)
        self.chunk_reads = chunk_reads(self.data, M.CHUNK)


@pytest.fixture(scope="module")
def the_file(tmp_path_factory):
    return TheFile(tmp_path_factory.mktemp("measure_cli"))


def run_cli(args, chunk=None, ok=True):
    env = {k: v for k, v in os.environ.items() if k != "TREW_MEASURE_CHUNK_BYTES"}
    if chunk is not None:
        env["TREW_MEASURE_CHUNK_BYTES"] = str(chunk)
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600, env=env)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def overflowing_chunks(f, name):
    """how many chunks hold more records of a logged measure than the first log of their batch takes (one record per read;
    chain: four events per read, and an item takes at least one event -- so for chain a lower bound; trace: sixteen items per
    read and motif and 1024 more, which no chunk of this file fills -- its workspace, a row per base and motif, none can)"""
    recs = f.host[name][0]
    per_read = [0] * len(f.reads)
    for r in recs["read"]:
        per_read[int(r)] += 1
    if name == "trace":
        return sum(1 for c in f.chunk_reads if sum(per_read[i] for i in c) > 16 * len(c) * len(M.MOTIFS) + 1024)
    room = 4 if name == "chain" else 1
    return sum(1 for c in f.chunk_reads if sum(per_read[i] for i in c) > room * len(c))


def test_the_file_and_its_borders_are_not_vacuous(the_file):
    """on the CPU, from chunk_spans and the expected records alone; first in the file, before anything is launched"""
    f = the_file
    assert 200_000 < len(f.data) < 600_000 and 550 <= len(f.reads) <= 650
    assert max(len(r) for r in f.reads) == 1500 and sum(1 for r in f.reads if not r) >= 3
    assert any(r != r.upper() for r in f.reads)
    quals = f.data.split(b"\n")[3::4]
    assert sum(1 for q in quals if q.startswith(b"@")) >= 50
    assert len(f.spans) >= 60
    batches = sum(1 for c in f.chunk_reads if c)
    assert len(chunk_spans(f.data, 1777)) > 2 * len(f.spans) and len(chunk_spans(f.data, 1 << 22)) == 2
    new_bytes = [off + carried for off, carried, _, _ in f.spans[1:]]
    behind_header = [b for b, (_, carried, num, _) in zip(new_bytes, f.spans[1:]) if num & 3 == 1 and carried == 0]
    at_sequence_newline = [b for b, (_, carried, num, _) in zip(new_bytes, f.spans[1:]) if num & 3 == 1 and f.data[b:b + 1] == b"\n"]
    assert behind_header and all(f.data[b - 1:b] == b"\n" for b in behind_header)
    assert at_sequence_newline and any(f.spans[1:][new_bytes.index(b)][1] > 0 for b in at_sequence_newline)
    for name in M.COMMANDS:
        reported = set(M.reported_reads(name, f.want[name]))
        assert len(reported) >= 150, name  # the planted reads
        assert 2 * sum(1 for c in f.chunk_reads if reported & set(c)) >= len(f.spans), name
        carried = sum(1 for (_, carried, _, _), c in zip(f.spans, f.chunk_reads) if carried > 0 and c and c[0] in reported)
        assert carried >= 10, name
    assert overflowing_chunks(f, "trace") == 0 and len(f.host["trace"][0]) > 16 * len(f.reads)
    for name in M.LOGGED:
        assert (0 < overflowing_chunks(f, name) or name == "trace") and sum(1 for c in f.chunk_reads if c and not any(int(r) in set(c) for r in f.host[name][0]["read"])) > 0, name
        if name != "chain":
            assert overflowing_chunks(f, name) < batches
    for name in ("periods", "repeats", "satellites", "refine", "tandems"):
        chunk_of = {i: n for n, c in enumerate(f.chunk_reads) for i in c}
        keys = M.summary_keys(name, f.want[name])
        assert len(f.want[name]) - f.want[name].index(">Summary") - 2 == len(keys) >= 3
        assert sum(1 for who in keys.values() if len({chunk_of[i] for i in who}) >= 2) >= 3, name
    assert any(k[0] == "171" for k in M.summary_keys("satellites", f.want["satellites"]))
    # rows of both motifs and both strands, so that no sort key of the merged rows is idle
    for name in ("annotate", "tracts", "intervals", "variants", "chain", "align", "trace"):
        rows = f.want[name][2:f.want[name].index(">Summary")]
        assert all(sum(1 for ln in rows if "," + m + "," in ln) >= 20 for m in M.MOTIFS), name
    for name in ("intervals", "chain", "align", "trace"):
        rows = f.want[name][2:f.want[name].index(">Summary")]
        assert all(sum(1 for ln in rows if "," + s + "," in ln) >= 20 for s in "+-"), name


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", M.COMMANDS)
def test_many_chunks_one_to_sixteen_workers(the_file, name, chunk):
    f = the_file
    for threads in THREADS:
        stats = ["--stats"] if threads == "4" else []
        r = run_cli(M.command_line(name, [f.path]) + ["-t", threads] + stats, chunk)
        assert r.stdout.splitlines() == f.want[name], (name, chunk, threads)
        if stats:
            batches = sum(1 for c in chunk_reads(f.data, chunk or 1 << 22) if c)
            assert "%d batch(es) submitted, chunk length %d bytes" % (batches, chunk or 1 << 22) in r.stderr
            if name in M.LOGGED and chunk == M.CHUNK:
                resubmitted = int(re.search(r"(\d+) batch\(es\) resubmitted with a larger log", r.stderr).group(1))
                assert 0 < resubmitted < batches or name == "trace", (name, resubmitted, batches)
                if name != "chain":
                    assert resubmitted == overflowing_chunks(f, name)
                else:
                    assert resubmitted >= overflowing_chunks(f, name)


@pytest.mark.parametrize("name", M.COMMANDS)
def test_gzip_and_bgzf_input(the_file, tmp_path, name):
    f = the_file
    gz, bgz = str(tmp_path / "single.fastq.gz"), str(tmp_path / "members.fastq.gz")
    with gzip.open(gz, "wb") as out:
        out.write(f.data)
    write_bgzf(bgz, f.data, block=777)
    for path in (gz, bgz):
        want = M.expected(name, [path], f.reads, f.host[name])
        assert run_cli(M.command_line(name, [path]) + ["-t", "4"], M.CHUNK).stdout.splitlines() == want, (name, path)


@pytest.mark.parametrize("name", M.COMMANDS)
def test_two_files_on_one_command_line(the_file, name):
    """the same file twice: the ordinals restart in the second section, the summary is over both"""
    f = the_file
    want = M.expected(name, [f.path, f.path], f.reads, f.host[name])
    assert want.count(want[0]) == 2
    assert run_cli(M.command_line(name, [f.path, f.path]) + ["-t", "4"], M.CHUNK).stdout.splitlines() == want


def test_crlf_line_ends(the_file, tmp_path):
    """every read one base longer: the carriage return matches nothing and counts towards the length, as in the reference
    reader and in the scan path"""
    data = the_file.data.replace(b"\n", b"\r\n")
    reads = M.reads_of(data)
    assert reads == [r + b"\r" for r in the_file.reads]
    path = str(tmp_path / "crlf.fastq")
    with open(path, "wb") as f:
        f.write(data)
    host = M.host_results(reads)
    for name in ("tracts", "periods"):
        want = M.expected(name, [path], reads, host[name])
        assert len(want) > 150
        assert run_cli(M.command_line(name, [path]) + ["-t", "4"], M.CHUNK).stdout.splitlines() == want, name


def test_a_read_that_does_not_fit_a_chunk(tmp_path):
    """at chunk 4096 a sequence line of 4094 bases behind a header whose newline is the first byte of a chunk ends the run
    with status 1, the message on stderr and an empty stdout; one of 4093 bases passes"""
    def fastq(n):
        seq = ("TTAGGG" * 700)[:n]
        return ("@" + "h" * (M.CHUNK - 2) + "\n" + seq + "\n+\n" + "I" * n + "\n@s\n" + "TTAGGG" * 10 + "\n+\n" + "I" * 60 + "\n").encode()
    path = str(tmp_path / "limit.fastq")
    with open(path, "wb") as f:
        f.write(fastq(M.CHUNK - 3))
    reads = M.reads_of(fastq(M.CHUNK - 3))
    assert [len(r) for r in reads] == [M.CHUNK - 3, 60]
    want = M.expected("tracts", [path], reads, M.host_results(reads)["tracts"])
    assert len(want) == 2 + 2 + 2 + 2
    assert run_cli(M.command_line("tracts", [path]) + ["-t", "4"], M.CHUNK).stdout.splitlines() == want
    with open(path, "wb") as f:
        f.write(fastq(M.CHUNK - 2))
    r = run_cli(M.command_line("tracts", [path]) + ["-t", "4"], M.CHUNK, ok=False)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "a read does not fit one %d-byte chunk\n" % M.CHUNK)
