"""GPU: the TOPP-RA kernels beyond one joint against something other than the oracle.  toppra_fast_kernel<1..7>,
toppra_wide_kernel<true / false> and toppra_sample_kernel are held to the exact stage certificate of tests/toppra_cert.py, to
scaled replicas of the reference's recorded 1-dof run, and to a dense-solve spline.  The bar for K, x, u, t is the 1e-9 the
kernels already keep against the oracle (test_toppra_matches_oracle); it rests on the oracle passing the same certificate at
1e-10 on the same plans, which tests/test_toppra_cert.py asserts without a GPU."""
import os

import numpy as np
import pytest

import toppra_cert as tc

pytestmark = pytest.mark.gpu
RTOL = 1e-5          # the bar on sampled profiles (BASELINE.json north_star)
CERT_TOL = 1e-9      # kernel against the certificate


@pytest.fixture(scope="module")
def ctx():
    import torch
    import sea_current_amd as sc
    assert torch.cuda.is_available()
    c = sc.Context(0)
    yield c
    c.close()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _solve(ctx, plans, N, sd_start=0.0, sd_end=0.0):
    """One batch through sc_toppra_hermite_batch -> (device outputs, per-plan numpy results)."""
    b = tc.stack(plans)
    out = ctx.toppra(*(_t(b[k]) for k in ("p0", "p1", "v0", "v1", "vlo", "vhi", "alo", "ahi")), N=N, sd_start=sd_start, sd_end=sd_end)
    ctx.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    return out, [dict(status=int(o["status"][p]), K=o["K"][p], x=o["x"][p], u=o["u"][p], t=o["t"][p]) for p in range(len(plans))]


def _sample(ctx, plans, out, dt, max_len):
    b = tc.stack(plans)
    smp = ctx.toppra_sample(*(_t(b[k]) for k in ("p0", "p1", "v0", "v1")), out["x"], out["t"], dt, max_len)
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in smp.items()}


def _oracle(oracle, pl, N, sd_start=0.0, sd_end=0.0):
    return oracle.toppra(pl["p0"], pl["p1"], pl["v0"], pl["v1"], pl["vlo"], pl["vhi"], pl["alo"], pl["ahi"], N=N,
                         sd_start=sd_start, sd_end=sd_end)


def _close(got, ref, tol=CERT_TOL):
    for k in ("K", "x", "u", "t"):
        assert np.max(np.abs(got[k] - ref[k])) <= tol * np.max(np.abs(ref[k])), k


CERT_SHAPES = ([(d, n, ps) for d, n in tc.FAST_SHAPES + tc.WIDE_SHAPES for ps in (0, 1)] +
               [(d, n, 1) for d, n in tc.WIDE_PER_STAGE_SHAPES])


@pytest.mark.parametrize("dof,N,per_stage", CERT_SHAPES)
def test_kernel_passes_certificate(ctx, oracle, dof, N, per_stage):
    """The kernel's own K, x, u, t against the definition.  Fast kernel: every template instance and every residue of N
    modulo its chunk of 4 stages, every stage certified.  Wide kernel: around its chunks of 32 stages, at most 12 stages a
    plan; per-stage limits at 16 joints on both sides of the point (N = 174 | 175) where they stop being staged in LDS."""
    plans, stages = tc.shape_plans(dof, N, per_stage)
    _, got = _solve(ctx, plans, N)
    for pl, st, g in zip(plans, stages, got):
        assert _oracle(oracle, pl, N)["status"] == 0 and g["status"] == 0
        res = tc.certify_plan(pl, N, g, stages=st)
        print(f"kernel certificate dof={dof} N={N} per_stage={per_stage}: {res:.2e}")
        assert res <= CERT_TOL


@pytest.mark.parametrize("dof,N", tc.MOVING_ENDS_SHAPES)
def test_kernel_passes_certificate_moving_ends(ctx, oracle, dof, N):
    """Plans that start and end in motion: x[0] = sd_start^2 inside K[0], K[N] = sd_end^2."""
    plans, stages = tc.shape_plans(dof, N, 1)
    _, got = _solve(ctx, plans, N, *tc.MOVING_ENDS)
    for pl, st, g in zip(plans, stages, got):
        assert _oracle(oracle, pl, N, *tc.MOVING_ENDS)["status"] == 0 and g["status"] == 0
        res = tc.certify_plan(pl, N, g, st, *tc.MOVING_ENDS)
        print(f"kernel certificate moving ends dof={dof} N={N}: {res:.2e}")
        assert res <= CERT_TOL


@pytest.mark.parametrize("dof,N", tc.SAMPLE_SHAPES)
def test_sample_kernel_matches_dense_spline(ctx, oracle, dof, N):
    """toppra_sample_kernel (shared pivots, reciprocals, knot compaction) against one dense fp64 solve of the same clamped
    spline through the kernel's own knots, at the kernel's own sample times."""
    plans, _ = tc.shape_plans(dof, N, 0)
    out, got = _solve(ctx, plans, N)
    s = _sample(ctx, plans, out, 0.02, 1024)
    for p, (pl, g) in enumerate(zip(plans, got)):
        assert g["status"] == 0 and np.diff(g["t"]).min() >= 1e-8
        T = g["t"][-1]
        n = int(s["length"][p])
        assert n == int(np.ceil(T / 0.02)) and 20 < n <= 1024
        assert np.allclose(s["time"][p, :n], tc.sample_times(T, 0.02), rtol=1e-12, atol=0)
        ref = tc.spline_reference(pl["p0"], pl["p1"], pl["v0"], pl["v1"], g["x"], g["t"], s["time"][p, :n])
        for k, q in zip(("pos", "vel", "acc"), ref):
            res = tc.sample_residual(s[k][p, :, :n], q)
            print(f"kernel sampling dof={dof} N={N} {k}: {res:.2e}")
            assert res < RTOL
            assert res < 2e-7


# ---- scaled replicas of the recorded run -----------------------------------------------------------------------------------

def _replica(oracle, golden_dir, c, slack):
    fx = np.load(os.path.join(golden_dir, "toppra_1dof_output.npz"))
    one = dict(p1=float(fx["arclength"]), v0=0.0, v1=0.0, vlo=float(fx["vel_lim"][0]), vhi=float(fx["vel_lim"][1]),
               alo=float(fx["acc_lim"][0]), ahi=float(fx["acc_lim"][1]))
    r1 = oracle.toppra([0.0], [one["p1"]], [0.0], [0.0], [one["vlo"]], [one["vhi"]], [one["alo"]], [one["ahi"]], N=100)
    assert r1["status"] == 0
    return fx, r1, tc.scaled_replica(c=c, slack=slack, **one)


@pytest.mark.parametrize("name", sorted(tc.REPLICAS))
def test_kernel_scaled_replicas_of_the_recording(ctx, oracle, golden_dir, name):
    """Joint k = the recorded 1-dof problem times c_k, through the fast (2, 3, 6, 7 joints) and the wide (8, 16) kernel: what
    test_toppra_fixture_1dof asserts of one joint, of every joint after dividing by c_k; K, x, u, t those of the 1-dof oracle."""
    c, slack, _ = tc.REPLICAS[name]
    fx, r1, pl = _replica(oracle, golden_dir, c, slack)
    out, (g,) = _solve(ctx, [pl], 100)
    assert g["status"] == 0
    _close(g, r1)
    assert np.float32(g["t"][-1]) == fx["time"][-1]
    s = _sample(ctx, [pl], out, float(np.float32(0.02)), 4400)
    n = int(s["length"][0])
    assert n == 4328
    assert np.array_equal(s["time"][0, :n].astype(np.float32), fx["time"])
    rel = lambda a, b: np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b))
    for k, ck in enumerate(c):
        vel, acc = s["vel"][0, k, :n].astype(np.float64), s["acc"][0, k, :n].astype(np.float64)
        if ck is tc.IDLE:
            assert not vel.any() and not acc.any()      # equal knot values: zero chord slopes, zero second derivatives
            continue
        print(f"kernel replica {name} joint {k}: vel {rel(vel / ck, fx['vel']):.2e} acc {rel(acc / ck, fx['acc']):.2e}")
        assert rel(vel / ck, fx["vel"]) < RTOL and rel(acc / ck, fx["acc"]) < RTOL, k
        assert rel(vel / ck, fx["vel"]) < 2e-7 and rel(acc / ck, fx["acc"]) < 2e-7, k
    res = tc.certify_plan(pl, 100, g, stages=tc.edge_stages(100, np.random.default_rng(3)))
    print(f"kernel certificate replica {name}: {res:.2e}")
    assert res <= CERT_TOL


def test_kernel_replica_joint_permutation(ctx, oracle, golden_dir):
    """The order of the joints decides which lane holds which row, nothing else."""
    c, slack, _ = tc.REPLICAS["dof6_general"]
    _, r1, pl = _replica(oracle, golden_dir, c, slack)
    perm = np.array([4, 2, 5, 0, 3, 1])
    _, (g, h) = _solve(ctx, [pl, {k: v[perm] for k, v in pl.items()}], 100)
    assert g["status"] == h["status"] == 0
    _close(g, r1)
    _close(h, r1)
    _close(h, g)


# ---- the zero-divisor pair beyond one joint --------------------------------------------------------------------------------

@pytest.mark.parametrize("dof", sorted(tc.ZERO_DIVISOR_SCALES))
def test_kernel_zero_divisor_pair_beyond_one_joint(ctx, oracle, dof):
    """The four plans of test_toppra_zero_divisor_pair as power-of-two scaled, sign-flipped copies of that joint plus an idle
    joint (fast kernel: the per-chunk flag with more than one slot; wide kernel: the alpha == 0 rule and cf == 0 pairs)."""
    z = tc.ZERO_DIVISOR
    N, sd = z["N"], z["sd"]
    plans = [tc.scaled_replica(z["p1"], z["v0"], z["v1"], -z["vl"], z["vl"], alo, ahi, tc.ZERO_DIVISOR_SCALES[dof])
             for alo, ahi in zip(z["alo"], z["ahi"])]
    _, got = _solve(ctx, plans, N, sd, sd)
    seen = set()
    for pl, g, alo, ahi in zip(plans, got, z["alo"], z["ahi"]):
        r1 = oracle.toppra([0.0], [z["p1"]], [z["v0"]], [z["v1"]], [-z["vl"]], [z["vl"]], [alo], [ahi], N=N, sd_start=sd, sd_end=sd)
        assert g["status"] == r1["status"]
        seen.add(g["status"])
        if r1["status"] == 0:
            _close(g, r1)
            res = tc.certify_plan(pl, N, g, sd_start=sd, sd_end=sd)
            print(f"kernel certificate zero divisor dof={dof}: {res:.2e}")
            assert res <= CERT_TOL
    assert 0 in seen and len(seen) > 1
