"""The host pipeline of the C++ drop-in (metamdbg_amd/host/mdbg_tool.cpp readSelection: parser workers -> consumers one batch ahead ->
record builders writing in place -> the statistics thread in read order -> the purge pass) driven on a CPU through thousands of
batches against a TEST DOUBLE of the library (tests/host/stub_mdbg_hip.cpp: fake minimizers that depend on the read's length only).
No GPU, no numerics -- order, completeness and freedom from deadlock, under several batch sizes, thread counts and timings: the output
must be the same bytes every time, and exactly what the fake minimizers imply.  (A missed wake-up between the consumers and the record
builders once hung the tool on a 50 Gbp file and took half an hour of GPU time to find out; this test reproduces it in a second.)"""
from __future__ import annotations

import os
import re
import struct
import subprocess

import numpy as np
import pytest

from metamdbg_amd import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def stub_tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("stubtool")
    lib = str(d / "libmdbg_hip.so")
    exe = str(d / "mdbg_tool")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host", "stub_mdbg_hip.cpp"), "-o", lib, "-lpthread"], check=True)
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "metamdbg_amd", "host", "mdbg_tool.cpp"), "-o", exe, "-L" + str(d), "-lmdbg_hip",
                    "-lz", "-lpthread", "-Wl,-rpath," + str(d)], check=True)
    return exe


@pytest.fixture(scope="module")
def read_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("stubreads")
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 4000, 30_000).astype(np.int64)
    lens[::97] = 0
    pool = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 200_000)]
    fasta = str(d / "reads.fasta")
    with open(fasta, "wb") as f:
        for i, n in enumerate(lens):
            a = int(rng.integers(0, len(pool) - 4000))
            f.write(b">r%d\n" % i + pool[a:a + int(n)].tobytes() + b"\n")
    # what the stub's fake minimizers imply for read_data_init.txt / read_data_corrected.txt
    init, corr = [], []
    for n in lens:
        L, k = int(n), int(n) // 271
        m = ((L * 2654435761 + np.arange(k, dtype=np.uint64) * 40503) & 0xFFFFFFFF).astype("<u4")
        init.append(struct.pack("<IB", k, 0) + m.tobytes() + (np.arange(k, dtype="<u4") * 271).astype("<u4").tobytes() +
                    ((L + np.arange(k)) & 1).astype("u1").tobytes() + np.ones(k, "u1").tobytes() + struct.pack("<II", 0xFFC00000, L))
        corr.append(struct.pack("<IB", k, 0) + m.tobytes())
    return fasta, b"".join(init), b"".join(corr), lens


@pytest.mark.parametrize("batch_bases,threads,jitter,ont,gpus,consumers", [
    (1 << 20, 32, 0, False, 1, 0), (1 << 20, 32, 30, False, 1, 0), (1 << 16, 8, 0, False, 1, 0), (1 << 18, 3, 100, False, 1, 0),
    (1 << 25, 16, 0, False, 1, 0), (1 << 14, 32, 0, False, 1, 0), (1 << 18, 16, 20, True, 1, 0), (1 << 15, 32, 0, True, 1, 0),
    # more than two consumers (round-3 ADVICE: both hung): --gpus 2 / 4 / 8 (two consumers per device from 8 threads up), MDBG_TOOL_CONSUMERS
    (1 << 15, 8, 0, False, 2, 0), (1 << 15, 8, 20, False, 6, 0), (1 << 15, 16, 0, False, 8, 0), (1 << 14, 8, 0, False, 8, 0),
    (1 << 15, 1, 0, False, 4, 0), (1 << 15, 10, 10, False, 8, 0), (1 << 15, 16, 0, False, 1, 3), (1 << 15, 16, 30, False, 1, 4),
    (1 << 15, 16, 10, True, 4, 0)])
def test_read_selection_pipeline_is_ordered_complete_and_does_not_hang(stub_tool, read_set, tmp_path, batch_bases, threads, jitter, ont, gpus, consumers):
    """ont: the ONT preset -- the census pre-pass (one batch ahead, ReadSelection.hpp:497-561) in front of the main pass, --skip-correction.
    gpus / consumers: several consumer threads (the test double has as many devices as it is asked for)."""
    fasta, exp_init, exp_corr, lens = read_set
    tmp = tmp_path / "out" / "tmp"
    os.makedirs(tmp / "filter")
    formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=not ont, data_type=1 if ont else 0,
                       correction_density=0.025).save(str(tmp / "parameters.gz"))
    (tmp / "input.txt").write_text(fasta + "\n")
    env = dict(os.environ, MDBG_STUB_JITTER_US=str(jitter), MDBG_TRACE="1")
    if consumers:
        env["MDBG_TOOL_CONSUMERS"] = str(consumers)
    for rep in range(3):
        r = subprocess.run([stub_tool, "readSelection", str(tmp), str(tmp / "read_data_init.txt"), str(tmp / "input.txt"), "--threads", str(threads),
                            "--min-read-quality", "0.000000", "--batch-bases", str(batch_bases), "--gpus", str(gpus)] + (["--skip-correction"] if ont else []),
                           env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-800:]
        assert (tmp / "read_data_init.txt").read_bytes() == exp_init
        assert (tmp / "read_data_corrected.txt").read_bytes() == exp_corr
        # the purge pass's group slabs: allocated beside the main pass when the input is many groups long, never more than wanted
        m = re.search(r"(\d+) of (\d+) group slabs were allocated beside the main pass", r.stderr)
        assert m, r.stderr[-800:]
        assert int(m.group(1)) <= int(m.group(2))
        assert (int(m.group(2)) > 0) == (os.path.getsize(fasta) // (batch_bases * 32) >= 2)
        st = formats.parse_read_stats((tmp / "read_stats.txt").read_bytes())
        assert st["n_reads"] == len(lens) and st["n_bases"] == int(lens.sum()) and st["n_minimizers"] == int((lens // 271).sum())


def test_pipeline_under_thread_sanitizer(read_set, tmp_path):
    """The same pipeline built with -fsanitize=thread (tool and test double): no data race between the feeder's workers, the consumers, the
    record builders, the statistics thread and the purge pass, in the HiFi and the ONT shape of the run."""
    fasta, exp_init, exp_corr, lens = read_set
    d = tmp_path / "tsan"
    os.makedirs(d)
    lib, exe = str(d / "libmdbg_hip.so"), str(d / "mdbg_tool")
    flags = ["-O1", "-g", "-fsanitize=thread", "-std=c++17"]
    r = subprocess.run(["g++"] + flags + ["-shared", "-fPIC", os.path.join(ROOT, "tests", "host", "stub_mdbg_hip.cpp"), "-o", lib, "-lpthread"], capture_output=True, text=True)
    if r.returncode == 0:
        r = subprocess.run(["g++"] + flags + [os.path.join(ROOT, "metamdbg_amd", "host", "mdbg_tool.cpp"), "-o", exe, "-L" + str(d), "-lmdbg_hip", "-lz", "-lpthread",
                            "-Wl,-rpath," + str(d)], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no ThreadSanitizer in this toolchain: " + r.stderr[-200:])
    for ont in (False, True):
        tmp = tmp_path / ("ont" if ont else "hifi") / "tmp"
        os.makedirs(tmp / "filter")
        formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=not ont, data_type=1 if ont else 0,
                           correction_density=0.025).save(str(tmp / "parameters.gz"))
        (tmp / "input.txt").write_text(fasta + "\n")
        r = subprocess.run([exe, "readSelection", str(tmp), str(tmp / "read_data_init.txt"), str(tmp / "input.txt"), "--threads", "16", "--min-read-quality", "0.000000",
                            "--batch-bases", str(1 << 17)] + (["--skip-correction"] if ont else []),
                           env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66"), capture_output=True, text=True, timeout=300)
        assert "ThreadSanitizer" not in r.stderr and r.returncode == 0, r.stderr[-1500:]
        assert (tmp / "read_data_init.txt").read_bytes() == exp_init and (tmp / "read_data_corrected.txt").read_bytes() == exp_corr
    # `graph --firstpass` over the file just written: four rank threads with a context each, then the pass in 7 pieces with the writer threads
    # of every share -- no report, the rows the test double implies
    os.makedirs(tmp / "smallContigs")
    counts = lens // 271
    exp_rec, exp_vec = _expected_first_pass(lens)
    for flags, extra in ((["--gpus", "4"], {}), ([], {"MDBG_TOOL_MAX_MINIMIZERS": str(_limit_for(counts, 7))})):
        r = subprocess.run([exe, "graph", str(tmp), "--threads", "16", "--min-abundance", "0", "--firstpass"] + flags,
                           env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66", MDBG_TOOL_NO_DETACH="1", **extra), capture_output=True, text=True, timeout=300)
        assert "ThreadSanitizer" not in r.stderr and r.returncode == 0, r.stderr[-1500:]
        assert (tmp / "kminmerData_abundance.txt").read_bytes() == (tmp / "kminmerData_abundance_init.txt").read_bytes() == exp_rec
        assert (tmp / "kminmerData_min.txt").read_bytes() == exp_vec


@pytest.mark.parametrize("batch_bases,threads,jitter,ont", [(1 << 18, 16, 0, False), (1 << 15, 8, 30, False), (1 << 16, 3, 0, False), (1 << 17, 16, 10, True), (1 << 25, 4, 0, False)])
def test_asm_step_is_the_two_commands_in_one_process(stub_tool, read_set, tmp_path, batch_bases, threads, jitter, ont):
    """`mdbg_tool asmStep` = readSelection + graph --firstpass in ONE process: the second command finds the library context alive and the
    corrected minimizers still on the device -- no second context, no read_data_corrected.txt parsed back (pipeline/AssemblyPipeline.hpp:716-740,
    :763-792 run them as two children).  Every file must be what the two commands write: read_data_init.txt, read_stats.txt and
    read_data_corrected.txt byte for byte, the tables as multisets (the first pass is handed the purged groups in the order they were purged
    in; the test double's rows are a function of the reads alone), the log lines of both, one perf.bin."""
    _asm_step_equals_the_two_commands(stub_tool, read_set, tmp_path, batch_bases, threads, jitter, ont)


def _asm_step_equals_the_two_commands(stub_tool, read_set, tmp_path, batch_bases, threads, jitter, ont, asm_step_env=None):
    """asm_step_env: what the asmStep run finds in its environment on top of the two commands'.  Returns the asmStep run's metaMDBG.log."""
    fasta, exp_init, exp_corr, lens = read_set
    P = formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=not ont, data_type=1 if ont else 0, correction_density=0.025)
    env = dict(os.environ, MDBG_STUB_JITTER_US=str(jitter))
    out = {}
    for mode in ("two", "one"):
        tmp = tmp_path / mode / "tmp"
        for d in ("filter", "smallContigs"):
            os.makedirs(tmp / d)
        P.save(str(tmp / "parameters.gz"))
        (tmp / "input.txt").write_text(fasta + "\n")
        rs = [str(tmp), str(tmp / "read_data_init.txt"), str(tmp / "input.txt"), "--threads", str(threads), "--min-read-quality", "0.000000",
              "--batch-bases", str(batch_bases)] + (["--skip-correction"] if ont else [])
        cmds = [[stub_tool, "readSelection"] + rs, [stub_tool, "graph", str(tmp), "--threads", str(threads), "--min-abundance", "0", "--firstpass"]] if mode == "two" \
            else [[stub_tool, "asmStep"] + rs + ["--min-abundance", "0"]]
        for cmd in cmds:
            r = subprocess.run(cmd, env=dict(env, **(asm_step_env or {})) if mode == "one" else env, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr[-800:]
        out[mode] = {n: (tmp / n).read_bytes() for n in ("read_data_init.txt", "read_data_corrected.txt", "read_stats.txt", "kminmerData_abundance.txt",
                                                          "kminmerData_abundance_init.txt", "kminmerData_min.txt", "perf.bin", "smallContigs/smallContigs_k4.bin")}
        out[mode]["log"] = (tmp_path / mode / "metaMDBG.log").read_text()
    one, two = out["one"], out["two"]
    assert one["read_data_init.txt"] == two["read_data_init.txt"] == exp_init
    assert one["read_data_corrected.txt"] == two["read_data_corrected.txt"] == exp_corr
    assert one["read_stats.txt"] == two["read_stats.txt"] and len(one["perf.bin"]) == 16 and one["smallContigs/smallContigs_k4.bin"] == b""
    n_rows = int((lens // 271 >= 4).sum())
    assert len(two["kminmerData_abundance.txt"]) == 20 * n_rows > 0
    for name, width in (("kminmerData_abundance.txt", 20), ("kminmerData_abundance_init.txt", 20), ("kminmerData_min.txt", 16)):
        a = np.frombuffer(one[name], np.uint8).reshape(-1, width)
        b = np.frombuffer(two[name], np.uint8).reshape(-1, width)
        assert a.shape == b.shape and np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])]), name
    assert one["kminmerData_abundance.txt"] == one["kminmerData_abundance_init.txt"]
    solid = [ln for ln in two["log"].splitlines() if "Nb solid kminmers" in ln or "Checksum kminmer abundance" in ln]
    assert len(solid) == 2 and [ln for ln in one["log"].splitlines() if "Nb solid kminmers" in ln or "Checksum kminmer abundance" in ln] == solid
    assert "mdbg_tool readSelection" in one["log"] and "mdbg_tool graph" in one["log"]
    return one["log"]


def test_asm_step_refuses_what_it_cannot_do(stub_tool, read_set, tmp_path):
    fasta = read_set[0]
    tmp = tmp_path / "x" / "tmp"
    os.makedirs(tmp / "filter")
    formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=False, data_type=1, correction_density=0.025).save(str(tmp / "parameters.gz"))
    (tmp / "input.txt").write_text(fasta + "\n")
    rs = [str(tmp), str(tmp / "read_data_init.txt"), str(tmp / "input.txt"), "--threads", "4", "--min-read-quality", "0.000000"]
    r = subprocess.run([stub_tool, "asmStep"] + rs, capture_output=True, text=True, timeout=60)          # ONT without --skip-correction: read correction lies in between
    assert r.returncode != 0 and "read correction" in r.stderr
    r = subprocess.run([stub_tool, "asmStep"] + rs + ["--skip-correction", "--gpus", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "one device" in r.stderr


# ---- `graph` through the test double: whole, in pieces, as ranks of a communicator ------------------------------------------------------------
# The double makes one row per read with at least k minimizers, in read order; pieces and ranks are contiguous read ranges written in order.
# So every way of running the first pass must write the same bytes, and they are known without running anything.

def _expected_first_pass(lens, k=4):
    """kminmerData_abundance.txt and kminmerData_min.txt as tests/host/stub_mdbg_hip.cpp's mdbg_kminmer_count_first implies them."""
    L = lens.astype(np.uint64)
    n = L // np.uint64(271)
    L, n = L[n >= k], n[n >= k]
    m = lambda i: (L * np.uint64(2654435761) + i * np.uint64(40503)) & np.uint64(0xFFFFFFFF)      # noqa: E731
    rec = np.zeros(len(L), dtype=[("lo", "<u8"), ("hi", "<u8"), ("ab", "<u4")])
    rec["lo"] = m(np.uint64(0)) | (m(np.uint64(1)) << np.uint64(32))
    with np.errstate(over="ignore"):
        rec["hi"] = m(n - np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + n
    rec["ab"] = n
    vec = np.stack([m(np.uint64(i)) for i in range(k)], axis=1).astype("<u4")
    return rec.tobytes(), vec.tobytes()


def _n_pieces(counts, limit):
    """The pieces `graph` cuts reads of `counts` minimizers into when one piece may hold `limit` (graph_plan.hpp, piece_cuts)."""
    pieces, held = 1, 0
    for c in counts:
        c = int(c)
        assert c <= limit
        if held + c > limit:
            pieces, held = pieces + 1, 0
        held += c
    return pieces


def _limit_for(counts, pieces):
    """A piece limit under which the read set takes exactly `pieces` pieces."""
    lo, hi = int(counts.max()), int(counts.sum())            # (the greedy cut is the fewest pieces: their number does not grow with the limit)
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if _n_pieces(counts, mid) <= pieces else (mid + 1, hi)
    assert _n_pieces(counts, lo) == pieces, (pieces, lo, _n_pieces(counts, lo))
    return lo


GRAPH_FILES = ("kminmerData_abundance.txt", "kminmerData_abundance_init.txt", "kminmerData_min.txt", "smallContigs/smallContigs_k4.bin", "perf.bin")
GRAPH_LOG_LINES = ("Checksum kminmer abundance", "Nb solid kminmers", "Nb rescued kminmers")


def _graph_first_pass(stub_tool, base, corrected, flags=(), env=None):
    """`graph --firstpass` over `corrected` as read_data_corrected.txt in base/tmp (made if need be; what is there stays): the finished process,
    the files it wrote and the log of the directory."""
    tmp = base / "tmp"
    os.makedirs(tmp / "smallContigs", exist_ok=True)
    formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=True, data_type=0, correction_density=0.025).save(str(tmp / "parameters.gz"))
    (tmp / "read_data_corrected.txt").write_bytes(corrected)
    r = subprocess.run([stub_tool, "graph", str(tmp), "--threads", "8", "--min-abundance", "0", "--firstpass"] + list(flags),
                       env=dict(os.environ, MDBG_TOOL_NO_DETACH="1", **(env or {})), capture_output=True, text=True, timeout=120)
    files = {n: (tmp / n).read_bytes() for n in GRAPH_FILES if (tmp / n).exists()}
    log = (base / "metaMDBG.log").read_text() if (base / "metaMDBG.log").exists() else ""
    return r, files, log


def _log_lines(log, what=GRAPH_LOG_LINES):
    return [ln for ln in log.splitlines() if any(w in ln for w in what)]


@pytest.fixture(scope="module")
def whole_graph(stub_tool, read_set, tmp_path_factory):
    """The first pass over the whole read set in one call: what every other way of running it must write."""
    r, files, log = _graph_first_pass(stub_tool, tmp_path_factory.mktemp("graphwhole"), read_set[2])
    assert r.returncode == 0, r.stderr[-800:]
    return files, log


def test_graph_whole_writes_what_the_double_implies(whole_graph, read_set):
    files, log = whole_graph
    exp_rec, exp_vec = _expected_first_pass(read_set[3])
    assert len(exp_rec) > 0 and set(files) == set(GRAPH_FILES)
    assert files["kminmerData_abundance.txt"] == files["kminmerData_abundance_init.txt"] == exp_rec and files["kminmerData_min.txt"] == exp_vec
    assert files["smallContigs/smallContigs_k4.bin"] == b"" and len(files["perf.bin"]) == 16
    assert len(_log_lines(log)) == 3 and "The pass runs in" not in log and "Self-check" not in log


def _same_as_whole(files, log, whole_graph):
    whole_files, whole_log = whole_graph
    assert set(files) == set(GRAPH_FILES)
    for name in GRAPH_FILES[:4]:
        assert files[name] == whole_files[name], name
    assert len(files["perf.bin"]) == 16
    assert _log_lines(log) == _log_lines(whole_log) and len(_log_lines(log)) == 3


@pytest.mark.parametrize("pieces", [2, 7, 64])
def test_graph_in_pieces_is_the_whole_pass(stub_tool, read_set, whole_graph, tmp_path, pieces):
    limit = _limit_for(read_set[3] // 271, pieces)
    r, files, log = _graph_first_pass(stub_tool, tmp_path, read_set[2], env={"MDBG_TOOL_MAX_MINIMIZERS": str(limit)})
    assert r.returncode == 0, r.stderr[-800:]
    _same_as_whole(files, log, whole_graph)
    assert "The pass runs in %d pieces of at most %d minimizers" % (pieces, limit) in log


@pytest.mark.parametrize("gpus,sharded_env", [(1, True), (3, False), (8, False)])
def test_graph_sharded_is_the_whole_pass(stub_tool, read_set, whole_graph, tmp_path, gpus, sharded_env):
    r, files, log = _graph_first_pass(stub_tool, tmp_path, read_set[2], flags=["--gpus", str(gpus)], env={"MDBG_TOOL_SHARDED": "1"} if sharded_env else None)
    assert r.returncode == 0, r.stderr[-800:]
    _same_as_whole(files, log, whole_graph)
    check = _log_lines(log, ("Self-check",))
    assert len(check) == 1 and "Self-check of the %d-rank table against the single-GPU pass: ok" % gpus in check[0]


def test_graph_no_verify_skips_the_self_check(stub_tool, read_set, whole_graph, tmp_path):
    r, files, log = _graph_first_pass(stub_tool, tmp_path, read_set[2], flags=["--gpus", "3", "--no-verify"])
    assert r.returncode == 0, r.stderr[-800:]
    _same_as_whole(files, log, whole_graph)
    assert "Self-check" not in log


def test_graph_refuses_a_read_above_the_limit_and_a_65th_piece(stub_tool, read_set, tmp_path):
    counts = read_set[3] // 271
    r, _, _ = _graph_first_pass(stub_tool, tmp_path / "read", read_set[2], env={"MDBG_TOOL_MAX_MINIMIZERS": str(int(counts.max()) - 1)})
    assert r.returncode != 0 and "one read has more minimizers than a piece may hold" in r.stderr
    r, _, _ = _graph_first_pass(stub_tool, tmp_path / "pieces", read_set[2], env={"MDBG_TOOL_MAX_MINIMIZERS": str(_limit_for(counts, 65))})
    assert r.returncode != 0 and "more than 64 pieces" in r.stderr


@pytest.mark.parametrize("pieces", [1, 7])
def test_graph_over_a_longer_table_leaves_files_of_the_new_length(stub_tool, read_set, tmp_path, pieces):
    """The table files are overwritten in place and cut to their length after the last write: a second pass over fewer reads into the same
    directory must leave the shorter table and nothing of the longer one behind it, whole and share by share."""
    corr, lens = read_set[2], read_set[3]
    counts = lens // 271
    few = len(lens) // 3
    short = corr[:5 * few + 4 * int(counts[:few].sum())]
    env = {"MDBG_TOOL_MAX_MINIMIZERS": str(_limit_for(counts[:few], pieces))} if pieces > 1 else None
    r, long_files, _ = _graph_first_pass(stub_tool, tmp_path, corr)
    assert r.returncode == 0, r.stderr[-800:]
    r, files, _ = _graph_first_pass(stub_tool, tmp_path, short, env=env)
    assert r.returncode == 0, r.stderr[-800:]
    exp_rec, exp_vec = _expected_first_pass(lens[:few])
    assert 0 < len(exp_rec) < len(long_files["kminmerData_abundance.txt"])
    assert files["kminmerData_abundance.txt"] == files["kminmerData_abundance_init.txt"] == exp_rec and files["kminmerData_min.txt"] == exp_vec


def test_asm_step_under_a_low_limit_runs_the_pass_in_pieces_from_the_file(stub_tool, read_set, tmp_path):
    """A piece limit below the read set's minimizers: asmStep drops the reads it holds on the device and its second command takes them from
    the file it has just written, in pieces -- and still writes what the two commands write."""
    limit = _limit_for(read_set[3] // 271, 5)
    log = _asm_step_equals_the_two_commands(stub_tool, read_set, tmp_path, 1 << 18, 16, 0, False, asm_step_env={"MDBG_TOOL_MAX_MINIMIZERS": str(limit)})
    assert "The pass runs in 5 pieces of at most %d minimizers" % limit in log
