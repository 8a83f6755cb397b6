"""MDBG_TOOL_DEVICE_RECORDS=1 against a library WITHOUT mdbg_minimizers_to_record_bytes (the CPU tests' double,
tests/host/stub_mdbg_hip.cpp): the symbol is looked up weakly, so the tool still links and starts, says on the MDBG_TRACE stream that
it takes the host builders, and writes the files it writes without the switch."""
from __future__ import annotations

import os
import subprocess

import numpy as np

from metamdbg_amd import formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_switch_without_the_symbol_takes_the_host_builders(tmp_path):
    lib, exe = str(tmp_path / "libmdbg_hip.so"), str(tmp_path / "mdbg_tool")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host", "stub_mdbg_hip.cpp"), "-o", lib, "-lpthread"], check=True)
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "metamdbg_amd", "host", "mdbg_tool.cpp"), "-o", exe, "-L" + str(tmp_path), "-lmdbg_hip",
                    "-lz", "-lpthread", "-Wl,-rpath," + str(tmp_path)], check=True)
    rng = np.random.default_rng(3)
    pool = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 100_000)]
    fasta = str(tmp_path / "reads.fasta")
    with open(fasta, "wb") as f:
        for i, n in enumerate(rng.integers(0, 4000, 3000)):
            a = int(rng.integers(0, len(pool) - 4000))
            f.write(b">r%d\n" % i + pool[a:a + int(n)].tobytes() + b"\n")
    outs = {}
    for name, env in (("off", {}), ("on", {"MDBG_TOOL_DEVICE_RECORDS": "1"})):
        tmp = tmp_path / name / "tmp"
        os.makedirs(tmp / "filter")
        formats.Parameters(minimizer_size=15, kminmer_size=4, density=0.005, first_k=4, prev_k=4, hpc=True, data_type=0).save(str(tmp / "parameters.gz"))
        (tmp / "input.txt").write_text(fasta + "\n")
        e = dict(os.environ, MDBG_TRACE="1")
        e.pop("MDBG_TOOL_DEVICE_RECORDS", None)
        e.update(env)
        r = subprocess.run([exe, "readSelection", str(tmp), str(tmp / "read_data_init.txt"), str(tmp / "input.txt"), "--threads", "8", "--min-read-quality", "0.000000",
                            "--batch-bases", str(1 << 16)], env=e, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-800:]
        if name == "on":
            assert "device records: falling back to the host builders" in r.stderr and "composed on the device" not in r.stderr
        else:
            assert "device records" not in r.stderr
        outs[name] = [(tmp / f).read_bytes() for f in ("read_data_init.txt", "read_data_corrected.txt", "read_stats.txt")]
    assert outs["on"] == outs["off"] and len(outs["off"][0]) > 13 * 3000
