"""The file path all fourteen per-read measures share (host/process.cpp: process_annotate, the serial chunk reader, the
workers' folds, add_totals and the sorts at the end) with many chunks a file: one generated FASTQ of a few hundred KB, cut
by TREW_MEASURE_CHUNK_BYTES into about a hundred (4096) or a few hundred (1777) batches that one, three or sixteen workers
share, must give byte for byte what the CPU definitions (capi.*_host) give over the whole file -- plain, gzip, BGZF, given
twice, with CRLF line ends -- and a read that does not fit a chunk must end the run cleanly.  Where the chunk borders
fall is taken from chunk_spans (tests/test_fastq_chunks_cpu.py, checked there against the product's reader).  decompose and
dissect print their signatures from the chunk's text and start their logs without slack, so most of their batches are
resubmitted; a second, small file of many tracts a read fills dissect's record log as well."""
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
        self.chunk_reads_1777 = chunk_reads(self.data, 1777)


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


def overflowing_chunks(f, name, chunks=None):
    """how many chunks hold more records of a logged measure than the first log of their batch takes (one record per read;
    chain: four events per read, and an item takes at least one event -- so for chain a lower bound; trace: sixteen items per
    read and motif and 1024 more, which no chunk of this file fills -- its workspace, a row per base and motif, none can;
    decompose: sixteen items per read; dissect: sixteen items per read, or four records per read and sixteen more).  chunks:
    the reads of every chunk at another chunk length than M.CHUNK"""
    if name in M.ITEMIZED:
        over_items, over_tracts = M.log_overflows(name, f.host[name], f.chunk_reads if chunks is None else chunks)
        return len(set(over_items) | set(over_tracts))
    assert chunks is None
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
    for name in ("periods", "repeats", "satellites", "refine", "tandems", "decompose", "dissect"):
        chunk_of = {i: n for n, c in enumerate(f.chunk_reads) for i in c}
        keys = M.summary_keys(name, f.want[name])
        assert len(f.want[name]) - f.want[name].index(">Summary") - 2 == len(keys) >= 3
        assert sum(1 for who in keys.values() if len({chunk_of[i] for i in who}) >= 2) >= 3, name
    assert any(k[0] == "171" for k in M.summary_keys("satellites", f.want["satellites"]))
    # rows of both motifs and both strands, so that no sort key of the merged rows is idle
    for name in ("annotate", "tracts", "intervals", "variants", "chain", "align", "trace"):
        rows = f.want[name][2:f.want[name].index(">Summary")]
        assert all(sum(1 for ln in rows if "," + m + "," in ln) >= 20 for m in M.MOTIFS), name
    for name in ("intervals", "chain", "align", "trace", "decompose", "dissect"):
        rows = f.want[name][2:f.want[name].index(">Summary")]
        assert all(sum(1 for ln in rows if "," + s + "," in ln) >= 20 for s in "+-"), name
    # decompose and dissect: the item log of most batches overflows and that of some does not, at both chunk lengths (measured:
    # 75 and 81 of 125 batches at 4096, 156 and 189 of 280 at 1777); the record log of dissect in none, a read of this file
    # has two tracts at the most (the second file is for that log)
    for name in M.ITEMIZED:
        for chunks in (f.chunk_reads, f.chunk_reads_1777):
            over_items, over_tracts = M.log_overflows(name, f.host[name], chunks)
            assert 2 * len(over_items) > sum(1 for c in chunks if c) > len(over_items) and not over_tracts, name
        rows = M.tract_rows(name, f.want[name])
        assert all(sum(1 for r in rows if r[3] == s) >= 20 for s in "+-"), name
        # tracts over a lowercase stretch of their read (measured: 13 and 16), printed from the chunk's text in upper case
        assert sum(1 for i, a, b, _, _ in rows if f.reads[i][a:b] != f.reads[i][a:b].upper()) >= 10, name
    rows = M.tract_rows("dissect", f.want["dissect"])
    assert all(a[0] < b[0] or (a[0] == b[0] and a[2] <= b[1]) for a, b in zip(rows, rows[1:]))  # sorted by (read, start), disjoint
    assert sum(1 for r in rows if any(c in "ACGT" for c in r[4])) >= 100  # an edited copy in the signature (measured: 298)
    per_read = {}
    for r in rows:
        per_read[r[0]] = per_read.get(r[0], 0) + 1
    assert sum(1 for v in per_read.values() if v == 2) >= 50 and max(per_read.values()) == 2  # (measured: 100 reads)
    # the --items forms: a row per item, many times the rows, and the tract column of dissect takes both values
    for name in M.ITEMIZED:
        want = M.expected(name, [f.path], f.reads, f.host[name], per_item=True)
        assert len(want) - want.index(">Summary") == len(f.want[name]) - f.want[name].index(">Summary")
        assert want.index(">Summary") - 2 == f.host[name][3 if name == "decompose" else 4] > 16 * (f.want[name].index(">Summary") - 2)
    assert {ln.split(",")[2] for ln in want[2:want.index(">Summary")]} == {"0", "1"}


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
            if name in M.ITEMIZED and chunk is not None:  # no slack in their logs: most batches, at both chunk lengths
                resubmitted = int(re.search(r"(\d+) batch\(es\) resubmitted with a larger log", r.stderr).group(1))
                assert 0 < resubmitted < batches, (name, resubmitted, batches)
                assert resubmitted == overflowing_chunks(f, name, f.chunk_reads if chunk == M.CHUNK else f.chunk_reads_1777)
            elif name in M.LOGGED and chunk == M.CHUNK:
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


@pytest.mark.parametrize("source", ["plain", "bgzf"])
@pytest.mark.parametrize("name", M.ITEMIZED)
def test_a_row_per_item(the_file, tmp_path, name, source):
    """decompose --items and dissect --items, three workers at chunk 4096: the items of a read carried over a chunk border
    keep the read's ordinal, and dissect's tract column counts within the read whatever the batch held in front of it"""
    f = the_file
    path = f.path
    if source == "bgzf":
        path = str(tmp_path / "members.fastq.gz")
        write_bgzf(path, f.data, block=777)
    want = M.expected(name, [path], f.reads, f.host[name], per_item=True)
    assert run_cli(M.command_line(name, [path], per_item=True) + ["-t", "4"], M.CHUNK).stdout.splitlines() == want


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
    for name in ("tracts", "periods", "decompose", "dissect"):
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


class TractFile:
    def __init__(self, folder):
        self.data = M.make_tract_file()
        self.reads = M.reads_of(self.data)
        packed = M.capi.pack_reads(self.reads)
        self.dissect = M.capi.dissect_host(packed)
        self.tandems = M.capi.tandems_host(packed)
        self.path = str(folder / "tracts.fastq")
        with open(self.path, "wb") as f:
            f.write(self.data)
        self.chunk_reads = chunk_reads(self.data, M.CHUNK)
        self.batches = sum(1 for c in self.chunk_reads if c)
        self.over_items, self.over_tracts = M.log_overflows("dissect", self.dissect, self.chunk_reads)


@pytest.fixture(scope="module")
def tract_file(tmp_path_factory):
    return TractFile(tmp_path_factory.mktemp("measure_cli_tracts"))


def test_the_second_file_fills_the_record_log_of_some_batches(tract_file):
    """on the CPU, from chunk_reads and the host definition alone (measured: 14, 14 and then 26, 10, 10 tracts a read as
    planted, depth up to 9; at chunk 4096 12 batches of 2 or 3 reads: the first over its record log alone, 8 over both logs,
    3 over their item log alone)"""
    f = tract_file
    assert len(f.reads) == M.TRACT_READS and 30_000 < len(f.data) < 50_000
    tracts = [int(v) for v in f.dissect[2][:, 0]]
    assert tracts[:2] == [M.CLEAN_TRACTS] * 2 and all(t >= (26 if i % 3 == 0 else 10) for i, t in enumerate(tracts[2:]))
    assert sum(tracts) == f.dissect[3] == f.tandems[2]
    assert int(f.dissect[0]["depth"].max()) >= 5
    assert f.batches >= 8 and {len(c) for c in f.chunk_reads if c} >= {2, 3}
    assert 3 <= len(f.over_tracts) < f.batches
    # every batch is resubmitted: the first for its records alone (as many items as tracts, or hardly more), some for their
    # items alone, the rest for both
    assert set(f.over_tracts) - set(f.over_items) == {0} and f.chunk_reads[0] == [0, 1]
    assert len(set(f.over_items) - set(f.over_tracts)) >= 2 and len(set(f.over_items) & set(f.over_tracts)) >= 3
    assert len(set(f.over_items) | set(f.over_tracts)) == f.batches
    per_read = [int(v) for v in f.tandems[1]]
    assert all(sum(per_read[i] for i in c) > len(c) for c in f.chunk_reads if c)  # tandems: a record per read


@pytest.mark.parametrize("per_item", [False, True], ids=["rows", "items"])
def test_many_tracts_a_read_fill_both_logs_of_dissect(tract_file, per_item):
    """one and three workers at chunk 4096; the batches resubmitted are the ones the CPU derives, and the retry takes the
    larger of the first room and the need in each of the two logs"""
    f = tract_file
    want = M.expected("dissect", [f.path], f.reads, f.dissect, per_item=per_item)
    assert want.index(">Summary") - 2 == f.dissect[4 if per_item else 3]
    for threads in ("2", "4"):
        r = run_cli(M.command_line("dissect", [f.path], per_item=per_item) + ["-t", threads, "--stats"], M.CHUNK)
        assert r.stdout.splitlines() == want, threads
        assert "%d batch(es) submitted, chunk length %d bytes" % (f.batches, M.CHUNK) in r.stderr
        resubmitted = int(re.search(r"(\d+) batch\(es\) resubmitted with a larger log", r.stderr).group(1))
        assert resubmitted == len(set(f.over_items) | set(f.over_tracts))


def test_many_tracts_a_read_through_tandems(tract_file):
    """the rows are the first columns of dissect's; the log starts at a record per read, so every batch is resubmitted"""
    f = tract_file
    want = M.expected("tandems", [f.path], f.reads, f.tandems)
    cut = len(M.tandem_ref.HEADER.split(","))
    rows = M.expected("dissect", [f.path], f.reads, f.dissect)
    assert [",".join(ln.split(",")[:cut]) for ln in rows[1:rows.index(">Summary")]] == want[1:want.index(">Summary")]
    for threads in ("2", "4"):
        r = run_cli(M.command_line("tandems", [f.path]) + ["-t", threads, "--stats"], M.CHUNK)
        assert r.stdout.splitlines() == want, threads
        resubmitted = int(re.search(r"(\d+) batch\(es\) resubmitted with a larger log", r.stderr).group(1))
        assert resubmitted == f.batches
