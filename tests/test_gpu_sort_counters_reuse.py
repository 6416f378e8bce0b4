"""A guard of behaviour the engine already had, kept while the timing events change their flags: one engine, two
workspace slots, the plan changing under the same slot from call to call -- a 2^12-point split MSM, 2^10 points, a
precomputed flat table, 2^13 points of another group, a batch that the device refuses (an index past the shared scalar
vector: AMDMSM_ERR_BAD_ARG after its kernels have run), then the 2^12-point MSM twice more.  Every result against the CPU
oracle.  With timing on, every ticket's phases are non-negative and sum to its total: the ring events are created with
hipEventDisableSystemFence (engine.cpp timing_event), and this is the test that reads them back across plans, slots and a
refused call.  It does not depend on how the sort's counters are cleared; nothing else of this file's subject is new.

The bound on that sum: the phases and the total are differences of the same six time stamps, each reported by
hipEventElapsedTime as a float of milliseconds "with a resolution of around 0.5 microseconds"; six values off by a quarter
of a microsecond each are 1.5 us, so 2 us."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import libff_amd  # noqa: E402
from libff_amd import OUT_AFFINE, multi_exp_base_form_special as SPECIAL  # noqa: E402

FLAT_C = 10
SUM_TOL_MS = 2e-3


@pytest.fixture(scope="module")
def eng():
    e = libff_amd.Engine(0, endomorphism=0)
    e.set_pipeline_depth(2)
    e.set_timing(True)
    yield e
    e.close()


def check_tickets(eng, first, last):
    """the timings of tickets first .. last"""
    for t in range(first, last + 1):
        ms = eng.get_timings(ticket=t)
        phases = [ms[k] for k in ("count_ms", "scatter_ms", "accumulate_ms", "reduce_ms", "final_ms")]
        assert all(p >= 0.0 for p in phases) and ms["total_ms"] > 0.0, (t, ms)
        assert abs(sum(phases) - ms["total_ms"]) <= SUM_TOL_MS, (t, ms)


def test_plans_change_under_the_same_slots(eng, port, tmp_path):
    def msm(curve, bases, sc):
        return np.asarray(port.multi_exp(curve, 1, bases, sc, port.BDLO12_SIGNED, port.FORM_SPECIAL, chunks=8, omp=True))

    b12, s12 = port.bases_seq(0, 1, 1 << 12, first=3), port.scalars_sha512(0, 11, 1 << 12)
    b10, s10 = port.bases_seq(0, 1, 1 << 10, first=4), port.scalars_sha512(0, 12, 1 << 10)
    bf, sf = port.bases_seq(0, 1, 700, first=5), port.scalars_sha512(0, 13, 700)
    b13, s13 = port.bases_seq(1, 1, 1 << 13, first=6), port.scalars_sha512(1, 14, 1 << 13)
    want12 = msm(0, b12, s12)
    assert libff_amd.plan(0, 1, 1 << 12, endomorphism=0)["endomorphism"]
    ticket = eng.last_timing_ticket()

    def timed(what):
        nonlocal ticket
        now = eng.last_timing_ticket()
        assert now > ticket, what
        check_tickets(eng, ticket + 1, now)
        ticket = now

    assert (eng.multi_exp(0, 1, b12, s12, base_form=SPECIAL) == want12).all()
    timed("2^12 split")
    assert (eng.multi_exp(0, 1, b10, s10, base_form=SPECIAL) == msm(0, b10, s10)).all()
    timed("2^10")
    tab = eng.precompute_table(0, 1, bf, FLAT_C)
    path = tmp_path / "table.bin"
    path.write_bytes(port.disk_write(0, 1, tab).tobytes())
    assert (eng.multi_exp_stream_with_precompute_file(0, 1, str(path), sf, FLAT_C) == msm(0, bf, sf)).all()
    timed("precomputed flat")
    assert (eng.multi_exp(1, 1, b13, s13, base_form=SPECIAL) == msm(1, b13, s13)).all()
    timed("2^13 bls12_377 G1")

    # a batch the device refuses: its sort, accumulation and tail have run in a slot when the flag is read
    aw = libff_amd.sizes(0, 1)["affine_bytes"] // 8
    idx = np.random.default_rng(2).integers(0, 600, size=1 << 12).astype(np.uint32)
    idx[2000] = 600
    shared = port.scalars_sha512(0, 15, 600)
    ptrs = []

    def put(arr):
        arr = np.ascontiguousarray(arr)
        p = eng.malloc(arr.nbytes)
        ptrs.append(p)
        eng.h2d(p, arr)
        return p.value

    try:
        d_b, d_sh, d_idx = put(b12[:, :aw]), put(shared), put(idx)
        d_out = put(np.zeros(libff_amd.sizes(0, 1)["g_bytes"] // 8, dtype=np.uint64))
        with pytest.raises(libff_amd.AmdMsmError, match="bad argument"):
            eng.msm_device_batch_items(0, 1, [dict(bases=d_b, n=1 << 12, index=d_idx, out=d_out)], d_sh, 600, out_form=OUT_AFFINE)
        eng.synchronize()
    finally:
        for p in ptrs:
            eng.free(p)
    now = eng.last_timing_ticket()
    check_tickets(eng, ticket + 1, now)   # whatever the refused call recorded is readable too
    ticket = now

    for rep in (1, 2):
        assert (eng.multi_exp(0, 1, b12, s12, base_form=SPECIAL) == want12).all(), rep
        timed(f"2^12 split again ({rep})")
