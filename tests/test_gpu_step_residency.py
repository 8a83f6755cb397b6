"""What every kernel of a device-sharing step needs of a compute unit against what the other context's 16-wave scan workgroup leaves of
it, from the loaded code object (mdbg_kernel_attributes = hipFuncGetAttributes).  A SIMD has 512 vector registers per
lane, allocated in eights, and eight wave slots; the scan holds four waves on each and 134 660 of a CU's 163 840 bytes of LDS.

LDS and wave slots are asserted for every kernel such a context launches.  Registers are asserted for every one of them EXCEPT the
three eight-wave split kernels listed below: they need 112 - 160 registers per lane where the scan leaves 96, the four-wave forms
("partition_threads" 256) that do fit were built for that reason -- and measured slower beside the scan, which got no faster
(profiles/split_residency_bench_alternating.txt).  So the exceptions are the shipped default, on purpose; the test pins that nothing
else joins them unnoticed, and that the four-wave forms keep fitting, so the comparison can be repeated.
GPU box: python -m pytest tests -m gpu"""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIMD_REGISTERS, REGISTER_GRANULE, SIMDS, CU_LDS, SCAN_WAVES_PER_SIMD = 512, 8, 4, 163840, 4
SCAN = "scan_prefiltered_16"


@pytest.fixture(scope="module")
def ctx():
    from metamdbg_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _allocated(registers):
    return (registers + REGISTER_GRANULE - 1) // REGISTER_GRANULE * REGISTER_GRANULE


def _waves_per_simd(threads):
    return ((threads + 63) // 64 + SIMDS - 1) // SIMDS


# over the register budget beside the scan, and the default all the same (see above)
REGISTER_EXCEPTIONS = {"split_hist_mins_512", "split_scatter_mins_512_tile2048", "split_scatter_records_512_tile2048"}
FOUR_WAVE_FORMS = ("split_hist_mins_256", "split_hist_records_256", "split_scatter_mins_256", "split_scatter_records_256")


def test_step_kernels_against_what_the_scan_leaves(ctx):
    names = ctx.step_kernel_names()
    attrs = {n: ctx.kernel_attributes(n) for n in names}
    scan = attrs[SCAN]
    assert scan["role"] == 0 and scan["threads"] == 1024 and scan["scratch"] == 0, scan
    # (a vector-register count: a workgroup of 16 waves could not be launched with more than 128)
    assert 64 <= scan["registers"] <= 128, scan
    registers_left = SIMD_REGISTERS - SCAN_WAVES_PER_SIMD * _allocated(scan["registers"])
    lds_left = CU_LDS - scan["static_lds"]
    slots_left = 8 - SCAN_WAVES_PER_SIMD
    assert registers_left > 0 and lds_left > 0, scan
    for n in names:
        a = attrs[n]
        print(f"{n:36s} threads {a['threads']:4d} registers {a['registers']:3d} need {_waves_per_simd(a['threads']) * _allocated(a['registers']):3d} of {registers_left} "
              f"lds {a['static_lds']:6d} of {lds_left} role {a['role']}")
    shared = [n for n in names if attrs[n]["role"] == 1]
    for wanted in ("split_hist_mins_512", "split_hist_records_512", "split_scatter_mins_512_tile2048", "split_scatter_records_512_tile2048",
                   "bucket_count_1024", "purge_detect", "purge_fix", "gather_prefix", "rescue_count", "emit_bucket_rows", "emit_rescued", "mark_starts",
                   "prefix_reduce", "prefix_apply"):
        assert wanted in shared, (wanted, shared)
    over_lds, over_slots, over_registers = [], [], set()
    for n in shared + list(FOUR_WAVE_FORMS):
        a = attrs[n]
        assert 0 < a["registers"] <= 512 and a["threads"] <= a["max_threads"] and a["scratch"] == 0, (n, a)
        wps = _waves_per_simd(a["threads"])
        if a["static_lds"] > lds_left:
            over_lds.append(n)
        if wps > slots_left:
            over_slots.append(n)
        if wps * _allocated(a["registers"]) > registers_left:
            over_registers.add(n)
    assert not over_lds and not over_slots, (over_lds, over_slots, lds_left)
    assert over_registers == REGISTER_EXCEPTIONS, (sorted(over_registers), registers_left)


def test_unknown_kernel_is_an_error(ctx):
    from metamdbg_amd import capi
    with pytest.raises(capi.MdbgError):
        ctx.kernel_attributes("no_such_kernel")


def test_default_context_keeps_the_eight_wave_split(ctx):
    """No shared options: the split kernels are the 512-thread, 4096-record ones, as before the four-wave forms existed."""
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 60, 500)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    mins = rng.integers(0, 25, int(offs[-1])).astype(np.uint32)
    ctx.set_option("first_pass_mode", 2)
    try:
        t = ctx.kminmer_count_first(ctx.minimizers_from_host(mins, offs), 4, 0)
        assert ctx.first_pass_info()["path"] == 2
        assert ctx.first_pass_form() == {"split_threads": 512, "split_tile": 4096}
        assert t.info()["n_records"] > 0
    finally:
        ctx.set_option("first_pass_mode", 0)
