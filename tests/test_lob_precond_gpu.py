"""MAC's preconditioned eigen-solver on the GPU (solver mode 2: precond.h, woodbury.h, solve_lob in solver_lob.h), pinned through the
iterations the library reports.

The preconditioner only proposes search directions: lambda_2, the Fiedler vector and the residual are decided by the sparse L(x),
so k_tri_band / k_tri_factor / k_tri_solve and their multi-workgroup forms, k_wb_extract / k_wb_cols / k_wb_big_* / k_wb_cap, the
Gauss-Jordan inverse k_gj_step, k_wb_g / k_wb_h / k_wb_w and k_lob_fused can be subtly wrong with every value right -- a stalled
solve is even handed to Lanczos, which returns the correct pair.  What a wrong preconditioner costs is iterations, and
`stats.lanczos_steps` counts them (the iterations the host had enqueued when the solve ended: a chunk end).

Reference: tests/lob_restatement.py, the same iteration and host schedule in NumPy with the plain preconditioner (a float64 inverse of
L + sigma I; LAPACK's banded solve of tridiag(L) + sigma I): J_ref.  Allowance: D / 4, two-sided (too few iterations means a stop
rule fired early), D the smallest excess of the damaged variants the case pins -- computed from the restatement, never from the
device.  tests/test_lob_precond_host.py asserts on the same inputs that D >= 8 and >= 0.1 J_ref, that rounding-size noise and the
device's own algebra stay within D / 8, and that every kernel has a pin of its own; it also lists what the counts cannot see.

Measured on the MI355X: every count of this module equals J_ref (8 to 224 iterations; deviation 0 on all ten pinned cases and
on intel, the smallest allowance 5), so the largest |deviation| / allowance is 0.000; the four mode / value cases, whose counts
are not asserted, agree with the restatement as well (6, 12, 109, 109).  lambda_2 against eigh / eigsh: 3.8e-8 relative at the
most (tri_n16385_s30, allowed 1e-6), 2.5e-9 or less on every exact-preconditioner case.  The fused and the look-ahead pairs
agree to the bit.
"""
import functools

import numpy as np
import pytest

import lob_restatement as Q
from mac_amd import _lib

pytestmark = pytest.mark.gpu

PINNED = [name for name, c in Q.cases().items() if c.pins]
VALUE_ONLY = [name for name, c in Q.cases().items() if not c.pins]


def problem_of(name, **opts):
    """The case as a handle forced into solver mode 2, with the case's options and `opts` on top."""
    c = Q.cases()[name]
    P = _lib.Problem(c.n, c.fi, c.fj, c.fw, c.ci, c.cj, c.cw)
    P.set_options(**{**c.options, **opts})
    P.set_start(c.start)
    P.set_solver(2)
    return P


def solve_on(P, name):
    P.set_x(Q.cases()[name].x)
    lam, v, _ = P.fiedler()
    return dict(lam=float(lam), steps=int(P.stats.lanczos_steps), restarts=int(P.stats.restarts), residual=float(P.stats.residual),
                mode=P.solve_mode(), vec=v)


def solve(name, **opts):
    P = problem_of(name, **opts)
    try:
        return solve_on(P, name)
    finally:
        P.close()


@functools.lru_cache(maxsize=None)
def lam_ref(name):
    return Q.lambda2_reference(Q.cases()[name])


def check_values(name, r):
    """Mode, closure count, restarts, residual, lambda_2 (1e-7 relative as test_exact_chain_plus_closures_preconditioner asks of the pose
    graphs; 1e-6, as the 200 000-node chain of test_gpu_parity.py, where lambda_2 < 1e-7 ||L||_inf)."""
    c, ref = Q.cases()[name], Q.reference(name)
    L = Q.laplacian(c)
    assert r["mode"] == ((7, ref["s"]) if c.exact else (6, 0))
    assert r["restarts"] == 0 and r["residual"] < 1e-8
    assert np.abs(L @ r["vec"] - r["lam"] * r["vec"]).sum() / Q.norm_inf(L) < 1e-8
    rtol = 1e-7 if lam_ref(name) >= 1e-7 * Q.norm_inf(L) else 1e-6
    print(f"{name}: mode {r['mode']}, lambda_2 {r['lam']!r} (reference {lam_ref(name)!r}, relative {abs(r['lam'] - lam_ref(name)) / lam_ref(name):.2e}, "
          f"allowed {rtol:.0e}), residual {r['residual']:.2e}")
    assert abs(r["lam"] - lam_ref(name)) <= rtol * lam_ref(name)


def check_count(name, r, tag=""):
    ref = Q.reference(name)
    dev, allow = r["steps"] - ref["J_ref"], ref["D"] / 4
    print(f"{name}{tag}: iterations {r['steps']}, J_ref {ref['J_ref']}, deviation {dev}, allowance {allow}, |deviation| / allowance {abs(dev) / allow:.3f}")
    assert abs(dev) <= allow


# ---- 1. every pinned case: values and the count ----
@pytest.mark.parametrize("name", PINNED)
def test_iterations_are_those_of_the_plain_preconditioner(name):
    r = solve(name)
    check_values(name, r)
    check_count(name, r)


# ---- 2. mode / value cases: s = 1, the two tiers, woodbury = 0 ----
@pytest.mark.parametrize("name", VALUE_ONLY)
def test_mode_and_values_where_counts_cannot_pin(name):
    r = solve(name)
    check_values(name, r)
    print(f"{name}: iterations {r['steps']} (restatement {Q.reference(name)['J_ref']}; not asserted: {Q.cases()[name].note})")


# ---- 3. option pairs on one input ----
def test_fused_update_gives_the_bits_of_the_three_kernels():
    """n = 4 096 (c = 4): k_lob_fused against k_lob_update + k_tri_solve + k_wb_g.  x, p, Lx, Lp, r and the solve are the same
    arithmetic per unknown in both, and the sums of the Rayleigh-Ritz step come from the product kernel either way; only the record
    ||r||_1 the host reads is added up in another order (per wave, then 16 totals, against per 256-thread workgroup), which moves
    its last bits and nothing the iterates are made of.  So: equal counts, equal lambda_2 bits, equal vectors."""
    (name, opts), = Q.PAIRS["lob_fuse"]
    a, b = solve(name), solve(name, **opts)
    for r, tag in ((a, " fused"), (b, " lob_fuse=0")):
        check_values(name, r)
        check_count(name, r, tag)
    assert a["steps"] == b["steps"] and a["lam"] == b["lam"] and np.array_equal(a["vec"], b["vec"])


@pytest.mark.parametrize("name,opts", Q.PAIRS["gj_look_min"])
def test_look_ahead_inverse_gives_the_bits_of_the_in_place_one(name, opts):
    """ld = 64, 128, 192 with gj_look_min = 64: the look-ahead route (pivot block inverted by the workgroup that holds it, one launch
    early; rotated tile grid) runs at 1, 2 and 3 tiles.  Both routes run gj_invert_block on the same stored values and the same
    products: equal counts and equal lambda_2 bits."""
    a, b = solve(name), solve(name, **opts)
    for r, tag in ((a, " in place"), (b, " look-ahead")):
        check_values(name, r)
        check_count(name, r, tag)
    assert a["steps"] == b["steps"] and a["lam"] == b["lam"] and np.array_equal(a["vec"], b["vec"])


# ---- 4. the counts are a function of the inputs ----
@pytest.mark.parametrize("name", ["n1025_s65_kinds", "tri_n2000_s30"])
def test_counts_repeat_on_the_same_handle_and_on_a_fresh_one(name):
    P = problem_of(name)
    try:
        first, again = solve_on(P, name), solve_on(P, name)
    finally:
        P.close()
    for r in (again, solve(name)):
        assert r["steps"] == first["steps"] and r["lam"] == first["lam"] and r["mode"] == first["mode"] and r["restarts"] == 0
        assert np.array_equal(r["vec"], first["vec"])
