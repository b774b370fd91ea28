"""host/fastq_chunks.hpp (the serial chunk reader of the `trew` host and the line location of its consumers) against
the reference reader's rule -- a sequence line is the line whose closing newline makes `num & 3 == 2`
(read_fastq_thread, kmer.cpp:987-1038) -- for chunk lengths that put a border at every byte position of a record, CRLF,
empty lines, header and quality lines longer than many chunks, files that do not end in a newline, and the longest
sequence line a chunk takes.  CPU only: the product's header is compiled with a small harness, once plain and once
with AddressSanitizer and UndefinedBehaviorSanitizer.

`chunk_spans` restates the border rule in Python; it is checked here against the product and is what
test_gpu_measure_cli.py derives its claims about borders from."""
import os
import subprocess

import pytest

from test_fastq_blocks_cpu import make_cases as block_cases, reference_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "harness", "chunks_harness.cpp")
DEFAULT_CHUNK = 1 << 22
MESSAGE = "a read does not fit one %d-byte chunk\n"


class ReadTooLong(Exception):
    pass


def chunk_spans(data: bytes, chunk: int):
    """The chunks the serial reader cuts `data` into: (offset, carried, num_before, total) each -- the file offset of the
    chunk's first byte, how many of its bytes were carried over from the chunk before (the begun sequence line), the
    newlines in front of it, its length.  A chunk holds at most chunk - 1 bytes; the read that returns nothing ends the
    file, so the last chunk holds only what was carried (usually nothing).  ReadTooLong where the reader gives up."""
    spans, pos, carried, num = [], 0, 0, 0
    while True:
        got = len(data[pos:pos + chunk - 1 - carried])
        offset, total = pos - carried, carried + got
        spans.append((offset, carried, num, total))
        num += data.count(b"\n", offset, offset + total)
        if got == 0:
            return spans
        pos += got
        carried = 0
        if num & 3 == 1:  # inside a sequence line
            carried = pos - (data.rfind(b"\n", offset, pos) + 1) if b"\n" in data[offset:pos] else total
            if carried >= chunk - 2:
                raise ReadTooLong()


def chunk_reads(data: bytes, chunk: int):
    """Per chunk of chunk_spans the ordinals of the sequence lines it reports: those whose closing newline lies in it."""
    lines, out, i = reference_rule(data), [], 0
    for offset, carried, num_before, total in chunk_spans(data, chunk):
        mine = []
        while i < len(lines) and lines[i][0] + lines[i][1] < offset + total:
            mine.append(i)
            i += 1
        out.append(mine)
    assert i == len(lines)
    return out


def fnv1a(b: bytes) -> int:
    h = 1469598103934665603
    for c in b:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def make_cases():
    cases = dict(block_cases())
    rec = "@r%d\n%s\n+\n%s\n"
    cases["header_and_quality_longer_than_chunks"] = "".join(
        "@" + "h" * (300 + 37 * i) + "\n" + "ACGTTGCA" * 5 + "\n+\n" + "@" + "I" * (450 + 41 * i) + "\n" for i in range(6)).encode()
    cases["empty_sequence_lines"] = ("".join(rec % (i, "" if i % 3 else "ACGTA"[:i % 5], "") for i in range(80)) + "@e\n\n+\n\n" * 40).encode()
    body = "".join(rec % (i, "ACGTN" * (i % 7), "I" * (5 * (i % 7))) for i in range(120))
    pad = -(len(body) + len("@p\nAC\n+\n\n")) % 63  # 63 = chunk - 1 at chunk 64, which the sweep below reaches (30 + 3 .. 30 + 70)
    cases["size_multiple_of_chunk_minus_1"] = (body + "@p\nAC\n+\n" + "I" * pad + "\n").encode()
    cases["size_multiple_of_chunk_minus_1_plus_one"] = (body + "@p\nAC\n+\n" + "I" * (pad + 1) + "\n").encode()
    assert len(cases["size_multiple_of_chunk_minus_1"]) % 63 == 0
    return cases


CASES = make_cases()


def build(exe, *flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, "-o", exe, SOURCE], capture_output=True, text=True)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("harness") / "chunks_harness")
    cc = build(exe)
    assert cc.returncode == 0, cc.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("harness") / "chunks_harness_asan")
    cc = build(exe, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if cc.returncode != 0:
        pytest.skip("AddressSanitizer runtime not available: " + cc.stderr[-200:])
    return exe


def run(exe, path, chunk, isa=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    if isa:
        env["TREW_SCAN_ISA"] = isa
    return subprocess.run([exe, path, str(chunk)], capture_output=True, text=True, env=env, timeout=300)


def expected_output(data, chunk, want):
    """What the harness prints: the chunks of chunk_spans, and every sequence line of the reference rule exactly once,
    in order, with its file-wide ordinal, its length and the hash of its bytes, under the chunk that holds its newline."""
    out = []
    for (offset, carried, num_before, total), mine in zip(chunk_spans(data, chunk), chunk_reads(data, chunk)):
        first = mine[0] if mine else (num_before + ((1 - num_before) & 3)) >> 2
        out.append("C %d %d %d %d" % (num_before, total, first, len(mine)))
        out += [want[i] for i in mine]
    return out


def sweep(exe, tmp_path, name, isas=()):
    data = CASES[name]
    path = str(tmp_path / "x.fastq")
    open(path, "wb").write(data)
    lines = reference_rule(data)
    want = ["L %d %d %016x" % (i, n, fnv1a(data[s:s + n])) for i, (s, n) in enumerate(lines)]
    longest = max([n for _, n in lines], default=0)
    chunks = list(range(longest + 3, longest + 71)) + [4096, 65536, DEFAULT_CHUNK]
    for chunk in chunks:
        r = run(exe, path, chunk)
        if chunk < longest + 2:  # 4096 on the long-line case: a line of chunk - 1 bytes or more never fits (test_the_limit)
            assert (r.returncode, r.stdout, r.stderr) == (1, "", MESSAGE % chunk), (name, chunk)
            continue
        assert r.returncode == 0 and r.stderr == "", (name, chunk, r.returncode, r.stderr[-2000:])
        got = r.stdout.splitlines()
        assert [x for x in got if x[0] == "L"] == want, (name, chunk)
        assert got == expected_output(data, chunk, want), (name, chunk)
    for isa in isas:  # the newline scan has an AVX2 form (the default, above), an opt-in AVX-512 form and a memchr form
        r = run(exe, path, longest + 40, isa)
        assert r.returncode == 0 and r.stdout.splitlines() == expected_output(data, longest + 40, want), (name, isa)


@pytest.mark.parametrize("name", sorted(CASES))
def test_chunks_find_the_reference_lines(harness, tmp_path, name):
    sweep(harness, tmp_path, name, isas=("avx512", "scalar"))


def test_sweep_puts_a_border_everywhere():
    """The sweep is not vacuous: over its chunk lengths the regular case sees a border directly behind a header's newline,
    directly in front of a sequence line's newline, inside every one of the four lines, and carried lines of many sizes."""
    data = CASES["regular"]
    seen, carried_sizes = set(), set()
    for chunk in range(403, 471):
        for offset, carried, num_before, total in chunk_spans(data, chunk)[1:]:
            border = offset + carried  # the first byte the chunk did not inherit
            seen.add((num_before & 3, "at_newline" if data[border:border + 1] == b"\n" else "behind_newline" if data[border - 1:border] == b"\n" else "inside"))
            carried_sizes.add(carried)
    for line in (0, 1, 3):  # (line 2 is the lone '+')
        assert (line, "inside") in seen, line
    for line in range(4):
        assert (line, "behind_newline") in seen and (line, "at_newline") in seen, line
    assert len(carried_sizes) > 100
    # the quality lines that start with '@' are cut as well, and the file of n (chunk - 1) bytes ends on a full read
    data = CASES["quality_starting_with_at"]
    assert any(num & 3 == 3 and data[off:off + 1] != b"@" and data[off - 1:off] != b"\n" for c in range(7, 75) for off, _, num, _ in chunk_spans(data, c)[1:])
    spans = chunk_spans(CASES["size_multiple_of_chunk_minus_1"], 64)
    assert spans[-1][3] == 0 and spans[-1][0] == len(CASES["size_multiple_of_chunk_minus_1"])


def limit_file(chunk, n, header=None):
    """A record whose sequence line has n bases behind a header of `header` bytes (default chunk - 1: the first chunk is
    the header, and the second begins with the header's newline), and a small record behind it."""
    header = chunk - 1 if header is None else header
    return ("@" + "h" * (header - 1) + "\n" + "ACGT" * (n // 4) + "ACGT"[:n % 4] + "\n+\n" + "I" * 5 + "\n@s\nTTAGGG\n+\nIIIIII\n").encode()


@pytest.mark.parametrize("chunk", [64, 4096])
def test_the_limit(harness, tmp_path, chunk):
    """A sequence line of chunk - 3 bytes passes wherever the borders fall; one of chunk - 2 bytes, with a border directly in
    front of its header's newline, and one of chunk - 1 bytes anywhere end with status 1, the message on stderr and
    nothing on stdout."""
    path = str(tmp_path / "x.fastq")
    for n, header, dies in [(chunk - 3, None, False), (chunk - 2, None, True)] + [(chunk - 3, h, False) for h in range(1, 70)] + [(chunk - 1, h, True) for h in range(1, 70)]:
        data = limit_file(chunk, n, header)
        open(path, "wb").write(data)
        r = run(harness, path, chunk)
        if dies:
            assert (r.returncode, r.stdout, r.stderr) == (1, "", MESSAGE % chunk), (n, header)
            with pytest.raises(ReadTooLong):
                chunk_spans(data, chunk)
        else:
            assert r.returncode == 0 and r.stderr == "", (n, header, r.stderr)
            lines = reference_rule(data)
            assert [x for x in r.stdout.splitlines() if x[0] == "L"] == ["L %d %d %016x" % (i, m, fnv1a(data[s:s + m])) for i, (s, m) in enumerate(lines)]
            assert lines[0][1] == n


@pytest.mark.parametrize("name", sorted(CASES))
def test_chunks_under_address_and_ub_sanitizer(sanitized, tmp_path, name):
    """The same sweep with -fsanitize=address,undefined (leak check on): every chunk is a malloc of exactly the chunk
    length, so a byte read or written past a chunk, a scratch array one slot short or a chunk nobody frees is a report."""
    sweep(sanitized, tmp_path, name)


def test_the_limit_under_address_and_ub_sanitizer(sanitized, tmp_path):
    path = str(tmp_path / "x.fastq")
    for n, dies in [(61, False), (62, True), (63, True), (200, True)]:
        open(path, "wb").write(limit_file(64, n))
        r = run(sanitized, path, 64)
        assert (r.returncode, r.stderr) == ((1, MESSAGE % 64) if dies else (0, "")), (n, r.stderr[-2000:])
        assert (r.stdout == "") == dies
