"""GPU parity: batched HIP TOPP-RA (through the C ABI) vs the CPU oracle and vs the reference's
recorded output.  Tolerance: north_star asks <= 1e-5 relative on velocity profiles; the kernel is
built with -ffp-contract=off and in practice agrees with the oracle to ~1e-12."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-5  # the bar (BASELINE.json north_star)


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


def test_toppra_fixture_1dof(ctx, oracle, golden_dir):
    import torch
    fx = np.load(os.path.join(golden_dir, "toppra_1dof_output.npz"))
    L = float(fx["arclength"])
    one = lambda v: _t([[v]])
    out = ctx.toppra(one(0.0), one(L), one(0.0), one(0.0), one(fx["vel_lim"][0]), one(fx["vel_lim"][1]),
                     one(fx["acc_lim"][0]), one(fx["acc_lim"][1]), N=100)
    torch.cuda.synchronize()
    assert int(out["status"][0]) == 0
    T = float(out["t"][0, -1])
    assert np.float32(T) == fx["time"][-1]
    dt = float(np.float32(0.02))
    smp = ctx.toppra_sample(one(0.0), one(L), one(0.0), one(0.0), out["x"], out["t"], dt, 4400)
    torch.cuda.synchronize()
    n = int(smp["length"][0])
    assert n == 4328
    rel = lambda a, b: np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b))
    assert np.array_equal(smp["time"][0, :n].cpu().numpy().astype(np.float32), fx["time"])
    assert rel(smp["vel"][0, 0, :n].cpu().numpy(), fx["vel"]) < RTOL
    assert rel(smp["acc"][0, 0, :n].cpu().numpy(), fx["acc"]) < RTOL
    assert rel(smp["vel"][0, 0, :n].cpu().numpy(), fx["vel"]) < 2e-7  # what we actually reach


@pytest.mark.parametrize("dof,N,P", [(1, 100, 8), (6, 200, 64), (3, 50, 16), (16, 64, 4)])
def test_toppra_matches_oracle(ctx, oracle, dof, N, P):
    import torch
    from sea_current_amd import synth
    pl = synth.toppra_plans(P, dof=dof)
    out = ctx.toppra(_t(pl["p0"]), _t(pl["p1"]), _t(pl["v0"]), _t(pl["v1"]), _t(-pl["vlim"]), _t(pl["vlim"]),
                     _t(-pl["alim"]), _t(pl["alim"]), N=N)
    smp = ctx.toppra_sample(_t(pl["p0"]), _t(pl["p1"]), _t(pl["v0"]), _t(pl["v1"]), out["x"], out["t"], 0.02, 1024)
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    s = {k: v.cpu().numpy() for k, v in smp.items()}
    for p in range(P):
        r = oracle.toppra(pl["p0"][p], pl["p1"][p], pl["v0"][p], pl["v1"][p], -pl["vlim"][p], pl["vlim"][p],
                          -pl["alim"][p], pl["alim"][p], N=N)
        assert o["status"][p] == r["status"] == 0
        for k in ("K", "x", "u", "t"):
            scale = np.max(np.abs(r[k])) + 1e-300
            assert np.max(np.abs(o[k][p] - r[k])) / scale < RTOL, (p, k)
            assert np.max(np.abs(o[k][p] - r[k])) / scale < 1e-9, (p, k)
        rs = oracle.toppra_sample(pl["p0"][p], pl["p1"][p], pl["v0"][p], pl["v1"][p], r["x"], r["t"], 0.02, 1024)
        n = rs["length"]
        assert s["length"][p] == n
        for k in ("pos", "vel", "acc"):
            scale = np.max(np.abs(rs[k])) + 1e-30
            assert np.max(np.abs(s[k][p, :, :n] - rs[k])) / scale < RTOL, (p, k)
        assert np.allclose(s["time"][p, :n], rs["time"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("N", [100, 2500])      # 2500 stages: the limits no longer fit in LDS (global-memory path)
def test_toppra_per_stage_limits(ctx, oracle, N):
    """Position-dependent velocity limits (LinearJointVelocityVarying, examples/test.cpp:194-213 style)."""
    import torch
    P, dof = 4, 2
    rng = np.random.default_rng(5)
    p0 = rng.uniform(-1, 1, (P, dof)); p1 = p0 + rng.uniform(1, 3, (P, dof))
    v0 = np.zeros((P, dof)); v1 = np.zeros((P, dof))
    s = np.arange(N + 1) / N
    vhi = 0.5 + 1.5 * np.abs(np.sin(3 * s))[None, :, None] * np.ones((P, 1, dof))
    al = np.full((P, dof), 2.0)
    out = ctx.toppra(_t(p0), _t(p1), _t(v0), _t(v1), _t(-vhi), _t(vhi), _t(-al), _t(al), N=N)
    torch.cuda.synchronize()
    for p in range(P):
        r = oracle.toppra(p0[p], p1[p], v0[p], v1[p], -vhi[p], vhi[p], -al[p], al[p], N=N)
        assert int(out["status"][p]) == r["status"] == 0
        assert np.allclose(out["x"][p].cpu().numpy(), r["x"], rtol=1e-9, atol=1e-12)
        assert np.allclose(out["t"][p].cpu().numpy(), r["t"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("per_stage", [0, 1])
def test_toppra_host_forms_equal_device_forms(ctx, per_stage):
    """sc_toppra_hermite_batch_host and sc_toppra_sample_batch_host (numpy through ctypes) give the bytes of the device forms
    on the same inputs: K, x, u, t and status whole, the samples as far as they are written (min(length, max_len))."""
    import sea_current_amd as sc
    from sea_current_amd import synth
    P, dof, N, L, dt = 12, 3, 60, 120, 0.02   # 67 .. 174 samples per plan
    pl = synth.toppra_plans(P, dof=dof)
    vlim = pl["vlim"]
    if per_stage:
        vlim = vlim[:, None, :] * (0.5 + np.abs(np.sin(3 * np.arange(N + 1) / N)))[None, :, None]
    a = lambda v: np.ascontiguousarray(v, dtype=np.float64)
    ends = [a(pl["p0"]), a(pl["p1"]), a(pl["v0"]), a(pl["v1"])]
    vl, al = [a(-vlim), a(vlim)], [a(-pl["alim"]), a(pl["alim"])]
    dev = ctx.toppra(*map(_t, ends + vl + al), N=N)
    ctx.synchronize()
    p = sc._ptr
    host = dict(K=np.empty((P, N + 1, 2)), x=np.empty((P, N + 1)), u=np.empty((P, N)), t=np.empty((P, N + 1)), status=np.empty(P, np.int32))
    assert sc.lib().sc_toppra_hermite_batch_host(ctx._h, P, dof, N, *map(p, ends + vl), per_stage, *map(p, al), 0.0, 0.0,
                                                 *[p(host[k]) for k in ("K", "x", "u", "t", "status")]) == 0
    for k in host:
        assert dev[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    assert (host["status"] == 0).all()
    smp = ctx.toppra_sample(*map(_t, ends), dev["x"], dev["t"], dt, L)
    ctx.synchronize()
    ds = {k: v.cpu().numpy() for k, v in smp.items()}
    hs = dict(pos=np.empty((P, dof, L), np.float32), vel=np.empty((P, dof, L), np.float32), acc=np.empty((P, dof, L), np.float32),
              time=np.empty((P, L)), length=np.empty(P, np.int32))
    assert sc.lib().sc_toppra_sample_batch_host(ctx._h, P, dof, N, *map(p, ends), p(host["x"]), p(host["t"]), dt, L,
                                                *[p(hs[k]) for k in ("pos", "vel", "acc", "time", "length")]) == 0
    assert ds["length"].tobytes() == hs["length"].tobytes()
    assert (hs["length"] > L).any() and (hs["length"] < L).any()      # plans cut at max_len and plans that end before it
    for q in range(P):
        n = min(int(hs["length"][q]), L)
        for k in ("pos", "vel", "acc"):
            assert ds[k][q, :, :n].tobytes() == hs[k][q, :, :n].tobytes(), (q, k)
        assert ds["time"][q, :n].tobytes() == hs["time"][q, :n].tobytes(), q


def test_toppra_statuses_match_oracle(ctx, oracle):
    """Plans the sweeps give up on (status 1: no controllable set; status 2: the start state is outside K[0]) next to
    solvable ones in one batch: statuses equal the oracle's, and whatever the oracle wrote before it stopped is there."""
    import torch
    N, dof = 60, 3
    rng = np.random.default_rng(9)
    P = 12
    p0 = rng.uniform(-1, 1, (P, dof)); p1 = p0 + rng.uniform(0.5, 2, (P, dof))
    v0 = rng.uniform(0.2, 1, (P, dof)); v1 = rng.uniform(0.2, 1, (P, dof))
    vl = np.full((P, dof), 2.0); al = np.full((P, dof), 3.0)
    alo = -al.copy(); ahi = al.copy()
    alo[1] = 1.0; ahi[1] = -1.0                      # empty acceleration interval: infeasible from the first stage
    alo[2, 1] = 0.5; ahi[2, 1] = 0.4                 # the same for one joint only
    vl[3] = 1e-3                                     # tiny velocity limits are fine (slow, feasible)
    sd_start, sd_end = 0.7, 0.1
    out = ctx.toppra(_t(p0), _t(p1), _t(v0), _t(v1), _t(-vl), _t(vl), _t(alo), _t(ahi), N=N, sd_start=sd_start, sd_end=sd_end)
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    seen = set()
    for p in range(P):
        r = oracle.toppra(p0[p], p1[p], v0[p], v1[p], -vl[p], vl[p], alo[p], ahi[p], N=N, sd_start=sd_start, sd_end=sd_end)
        assert o["status"][p] == r["status"], p
        seen.add(int(r["status"]))
        if r["status"] == 0:
            for k in ("K", "x", "u", "t"):
                assert np.allclose(o[k][p], r[k], rtol=1e-9, atol=1e-12), (p, k)
        assert np.allclose(o["K"][p, N], r["K"][N], rtol=0, atol=0)
    assert {0, 1, 2} <= seen or {0, 1} <= seen


def test_toppra_zero_divisor_pair(ctx, oracle):
    """A stage where a row pair's divisor is exactly zero (alpha_lower = 2 Delta beta_lower): that pair bounds nothing, but
    decides feasibility by its right-hand side -- the branch the fast kernel handles apart from its quotients."""
    import torch
    N = 4                                            # Delta = 0.25 exactly
    # c1 = 0.5, c2 = 1, c3 = 0: a(s) = 0.5 + 2 s, b = 2; at s = 0.25 the collocation slot has a = 1 = 2 Delta b
    p0 = np.zeros((4, 1)); p1 = np.full((4, 1), 1.5)
    v0 = np.full((4, 1), 0.5); v1 = np.full((4, 1), 2.5)
    vl = np.full((4, 1), 50.0)
    alo = np.array([[-4.0], [0.5], [1.0], [-40.0]]); ahi = np.array([[4.0], [4.0], [4.0], [40.0]])
    out = ctx.toppra(_t(p0), _t(p1), _t(v0), _t(v1), _t(-vl), _t(vl), _t(alo), _t(ahi), N=N, sd_start=0.5, sd_end=0.5)
    torch.cuda.synchronize()
    for p in range(4):
        r = oracle.toppra(p0[p], p1[p], v0[p], v1[p], -vl[p], vl[p], alo[p], ahi[p], N=N, sd_start=0.5, sd_end=0.5)
        assert int(out["status"][p]) == r["status"], p
        if r["status"] == 0:
            for k in ("K", "x", "u", "t"):
                assert np.allclose(out[k][p].cpu().numpy(), r[k], rtol=1e-9, atol=1e-12), (p, k)
