"""The phase contract of include/amdmsm.h where the marks of the Fr entries come from one skeleton (engine.cpp fr_call):
a timed host call reports the upload, the kernels and the download, a timed device call the kernels alone, every call
takes a ticket of its own, and an untimed call still computes what the models say.  One field, bls12_377."""
import numpy as np
import pytest

import fr_fft_model as fft_model
import fr_matrix_model as matrix_model
import fr_scan_model as scan_model
from fr_dev import Dev

pytestmark = pytest.mark.gpu

from libff_amd import plan_fr_fft, plan_fr_scan  # noqa: E402

CURVE = 1


def families(engine, stack):
    """(name, host call, device call, expected records) of the three families; the calls return records"""
    f = fft_model.field(CURVE)
    rec = f.limbs * 8
    out = []

    def device(run, recs, n_out):
        d = stack[0]
        d_in, d_out = d.up(recs), d.buf(n_out * rec)
        return lambda: (run(d_in, d_out), d.down(d_out, (n_out, f.limbs)))[1]

    n = 1 << 11
    assert plan_fr_fft(CURVE, n)["passes"] == 2   # at the default tile
    a = fft_model.random_vector(CURVE, n)
    recs = f.records(a, False)
    out.append(("fr_fft", lambda: engine.fr_fft(CURVE, recs), device(lambda i, o: engine.fr_fft_device(CURVE, i, n, o), recs, n),
                f.records(fft_model.fft(a, f.root(n), f.r), False)))

    m = matrix_model.random_matrix(f.r, [(7 * i) % 12 for i in range(40)], 30, seed=3)
    x = matrix_model.random_x(f.r, 30, seed=4)
    xr = f.records(x, False)
    mat = engine.fr_matrix_load(CURVE, *m.arrays(f, False), m.n_cols)
    stack.append(mat)
    out.append(("fr_matrix_apply", lambda: engine.fr_matrix_apply(mat, xr),
                device(lambda i, o: engine.fr_matrix_apply_device(mat, i, 30, o, 40), xr, 40), f.records(matrix_model.apply(m, x, f.r), False)))

    k = plan_fr_scan(CURVE, 0, invert=True)["tile"] + 3   # one default tile and three records
    base = [0] + scan_model.random_vector(CURVE, 498, seed=5)
    v = [base[(i * i + i // 3) % 499] for i in range(k)]
    vr = f.records(v, False)
    out.append(("fr_batch_invert", lambda: engine.fr_batch_invert(CURVE, vr)[0],
                device(lambda i, o: engine.fr_batch_invert_device(CURVE, k, i, o), vr, k), f.records(scan_model.invert(f.r, v)[0], False)))
    return out


def test_phases_tickets_and_the_untimed_path(engine):
    with Dev(engine) as d:
        stack = [d]
        try:
            cases = families(engine, stack)
            engine.set_timing(True)
            last = engine.last_timing_ticket()
            for name, host, device, want in cases:
                assert (host() == want).all(), name
                ticket = engine.last_timing_ticket()
                t = engine.get_timings(ticket=ticket)
                print(name, "host", ticket, t)
                assert ticket != last, name
                assert t["scatter_ms"] > 0 and t["count_ms"] >= 0 and t["accumulate_ms"] >= 0, (name, t)
                assert t["total_ms"] >= t["scatter_ms"], (name, t)
                last = ticket
                assert (device() == want).all(), name
                ticket = engine.last_timing_ticket()
                t = engine.get_timings(ticket=ticket)
                print(name, "device", ticket, t)
                assert ticket != last, name
                assert t["scatter_ms"] > 0 and t["accumulate_ms"] == 0, (name, t)
                last = ticket
            engine.set_timing(False)   # no events are recorded, and the slot's timings are no longer valid
            for name, host, device, want in cases:
                assert (host() == want).all() and (device() == want).all(), name
        finally:
            engine.set_timing(False)
            for mat in stack[1:]:
                mat.free()
