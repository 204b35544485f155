"""GPU parity: HIP EDT (through the C ABI) vs the CPU oracle, bit-exact int32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    import sea_current_amd as sc
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = sc.Context(0)
    yield c
    c.close()


def _gpu_edt(ctx, occ):
    import torch
    d = ctx.edt(torch.from_numpy(np.ascontiguousarray(occ)).cuda())
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize("W,H,p", [(1, 1, 0.5), (5, 3, 0.4), (16, 16, 0.1), (64, 64, 0.2), (33, 65, 0.05),
                                   (100, 37, 0.02), (256, 256, 0.05), (250, 130, 0.3), (1024, 96, 0.001)])
def test_edt_matches_oracle_random(ctx, oracle, W, H, p):
    rng = np.random.default_rng(W * 7919 + H)
    occ = (rng.random((H, W)) < p).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8)
    assert np.array_equal(_gpu_edt(ctx, occ), oracle.edt(occ))


def test_edt_edge_cases(ctx, oracle):
    import sea_current_amd as sc
    assert np.all(_gpu_edt(ctx, np.zeros((70, 40), np.uint8)) == sc.EDT_INF)      # empty grid
    assert np.all(_gpu_edt(ctx, np.ones((70, 40), np.uint8)) == 0)                # full grid
    occ = np.zeros((200, 300), np.uint8); occ[199, 0] = 7                        # one far corner obstacle
    assert np.array_equal(_gpu_edt(ctx, occ), oracle.edt(occ))
    occ = np.zeros((1, 2000), np.uint8); occ[0, 1999] = 1                        # single row
    assert np.array_equal(_gpu_edt(ctx, occ), oracle.edt(occ))
    occ = np.zeros((2000, 1), np.uint8); occ[3, 0] = 1                           # single column
    assert np.array_equal(_gpu_edt(ctx, occ), oracle.edt(occ))
    # sparse grids on every kernel variant (W = 1024 full-width fast path, ragged W, wide W):
    # distances beyond 255 force the 32-bit fallback rows
    for (H, W) in ((40, 1024), (70, 600), (300, 400), (40, 2048), (33, 3000)):
        assert np.all(_gpu_edt(ctx, np.zeros((H, W), np.uint8)) == sc.EDT_INF), (H, W)
        occ = np.zeros((H, W), np.uint8); occ[H // 3, W - 7] = 1
        assert np.array_equal(_gpu_edt(ctx, occ), oracle.edt(occ)), (H, W)
        occ[H - 1, 2] = 1; occ[0, W // 2] = 9
        assert np.array_equal(_gpu_edt(ctx, occ), oracle.edt(occ)), (H, W)
    occ = np.zeros((700, 1024), np.uint8); occ[350, 500:520] = 1                 # vertical distances > 255
    assert np.array_equal(_gpu_edt(ctx, occ), oracle.edt(occ))


def test_edt_batch_and_blocks(ctx, oracle):
    import torch
    from sea_current_amd import synth
    grids = np.stack([synth.block_grid(192, 160, 0.2, seed=s, smin=3, smax=30) for s in range(5)]
                     + [synth.salt_grid(192, 160, 0.05, seed=9)])
    d = ctx.edt(torch.from_numpy(grids).cuda()).cpu().numpy()
    for i in range(grids.shape[0]):
        assert np.array_equal(d[i], oracle.edt(grids[i])), i


def test_edt_1024_bench_grids(ctx, oracle):
    from sea_current_amd import synth
    for occ in (synth.salt_grid(1024, 1024, 0.05), synth.salt_grid(1024, 1024, 0.20), synth.block_grid(1024, 1024, 0.2)):
        assert np.array_equal(_gpu_edt(ctx, occ), oracle.edt(occ))


def test_edt_host_entry_point(ctx, oracle):
    from sea_current_amd import synth
    occ = synth.salt_grid(130, 70, 0.1, seed=4)
    assert np.array_equal(ctx.edt_host(occ), oracle.edt(occ))


def test_edt_4096_properties(ctx):
    """Full-size check through size-independent properties: d2 == 0 exactly on obstacles,
    1-Lipschitz in distance (|sqrt d2| differs by <= 1 between 4-neighbours), and agreement with
    the oracle on random row windows is covered at 1024^2; here we also spot-check cells by brute force."""
    import torch
    from sea_current_amd import synth
    occ = synth.salt_grid(4096, 4096, 0.01, seed=2)
    d2 = _gpu_edt(ctx, occ)
    assert np.array_equal(d2 == 0, occ != 0)
    d = np.sqrt(d2.astype(np.float64))
    assert np.abs(np.diff(d, axis=0)).max() <= 1 + 1e-9 and np.abs(np.diff(d, axis=1)).max() <= 1 + 1e-9
    ys, xs = np.nonzero(occ)
    rng = np.random.default_rng(0)
    for _ in range(200):
        y, x = rng.integers(0, 4096, 2)
        m = (np.abs(ys - y) <= 64) & (np.abs(xs - x) <= 64)
        assert d2[y, x] == ((ys[m] - y) ** 2 + (xs[m] - x) ** 2).min()


def test_edt_nearest_matches_oracle(ctx, oracle):
    import torch
    from sea_current_amd import synth
    grids = [synth.salt_grid(97, 61, 0.05, seed=4), synth.salt_grid(64, 64, 0.3, seed=5), synth.block_grid(200, 150, 0.2, seed=6, smin=3, smax=30),
             np.zeros((33, 47), np.uint8)]
    grids[3][10, 10] = 1
    for occ in grids:
        o = torch.from_numpy(occ).cuda()
        d2 = ctx.edt(o)
        nn = ctx.edt_nearest(o, d2)
        torch.cuda.synchronize()
        assert np.array_equal(nn.cpu().numpy(), oracle.edt_nearest(occ, oracle.edt(occ)))
    occ = synth.salt_grid(48, 40, 0.1, seed=7)
    nn = ctx.edt_nearest(torch.from_numpy(occ).cuda(), ctx.edt(torch.from_numpy(occ).cuda()))
    assert np.array_equal(nn.cpu().numpy(), oracle.edt_nearest(occ))            # against the exhaustive definition
    empty = torch.zeros((2, 16, 16), dtype=torch.uint8, device="cuda")
    assert (ctx.edt_nearest(empty, ctx.edt(empty)) == -1).all()
    big = synth.salt_grid(1024, 1024, 0.2)
    ob = torch.from_numpy(np.stack([big, synth.block_grid(1024, 1024, 0.2)])).cuda()
    d2b = ctx.edt(ob)
    nb = ctx.edt_nearest(ob, d2b).cpu().numpy()
    for k in range(2):
        assert np.array_equal(nb[k], oracle.edt_nearest(ob[k].cpu().numpy(), d2b[k].cpu().numpy()))


@pytest.mark.parametrize("W,H", [(1025, 40), (1984, 33), (2049, 70), (3000, 64), (3073, 17), (4095, 31), (4096, 50), (5000, 40),
                                 (4097, 33), (6145, 17), (8192, 33)])
def test_edt_wide_rows(ctx, oracle, W, H):
    """Rows of 1025 .. 4096 pixels run whole in registers (edt_band_wide_kernel: 16-row groups, producer / consumer
    wavefronts); rows its packed cascade cannot settle (distances beyond 175 columns) are redone in 32 bits inside the same
    launch; wider rows still go through 1024-column windows (the last four shapes: the narrowest such width, an odd one,
    and the full width with a partial second band, whose whole-row pass is edt_band_kernel<128, true>).  One batch mixes
    dense, sparse, seam and empty grids, which between them need all three passes of the window route."""
    import torch
    rng = np.random.default_rng(W)
    dense = (rng.random((H, W)) < 0.2).astype(np.uint8)
    sparse = (rng.random((H, W)) < 2e-4).astype(np.uint8)             # distances of hundreds of columns
    edge = np.zeros((H, W), np.uint8); edge[:, 959:962] = 1; edge[H // 2, W - 1] = 1   # obstacles at a 1024-column seam
    empty = np.zeros((H, W), np.uint8)
    occ = np.stack([dense, sparse, edge, empty, dense[::-1].copy()])
    d2 = ctx.edt(torch.from_numpy(occ).cuda())
    torch.cuda.synchronize()
    got = d2.cpu().numpy()
    for b in range(occ.shape[0]):
        assert np.array_equal(got[b], oracle.edt(occ[b])), b


@pytest.mark.parametrize("W", [100, 300, 1000, 2000, 5000])
def test_edt_timing_brackets(oracle, W):
    """Launch timing of one EDT on a fresh context, on every route of the dispatch: one colbits bracket and one band bracket
    (edt_updown_kernel counts as band time), three band brackets for rows wider than 4096 (two window passes and the
    whole-row pass).  With timing switched off again, further EDTs -- the routes that open their bracket ahead of a second
    launch included -- add nothing and raise nothing."""
    import torch
    import sea_current_amd as sc
    from sea_current_amd import synth
    H = 40
    occ = synth.salt_grid(W, H, 0.1, seed=W)
    c = sc.Context(0)
    c.set_timing(True)
    d2 = c.edt(torch.from_numpy(occ).cuda())
    c.synchronize()
    ms_c, n_c = c.get_timing(sc.K_EDT_COLBITS)
    ms_b, n_b = c.get_timing(sc.K_EDT_BAND)
    print(f"W={W}: colbits {n_c} x, {ms_c:.4f} ms; band {n_b} x, {ms_b:.4f} ms")
    assert n_c == 1
    assert n_b == (3 if W > 4096 else 1)
    assert ms_c > 0 and ms_b > 0
    assert np.array_equal(d2.cpu().numpy(), oracle.edt(occ))
    c.set_timing(False)
    for W2 in (2000, 5000):
        occ2 = synth.salt_grid(W2, H, 0.1, seed=W2)
        d2 = c.edt(torch.from_numpy(occ2).cuda())
        c.synchronize()
        assert np.array_equal(d2.cpu().numpy(), oracle.edt(occ2))
    assert c.get_timing(sc.K_EDT_COLBITS) == (ms_c, n_c)
    assert c.get_timing(sc.K_EDT_BAND) == (ms_b, n_b)
    c.close()


@pytest.mark.parametrize("W", [2048, 3100, 4096])
def test_edt_wide_rows_packed_range_boundary(ctx, oracle, W):
    """Free stretches whose half-width straddles what the packed cascade can represent (176 columns, distance bytes clamped
    at 177): walls 2 d + 1 columns apart leave d free columns either side of the middle, with d from 168 to 184, in rows
    far from any other obstacle; plus vertical distances around the clamp."""
    import torch
    H = 420
    occ = np.zeros((H, W), np.uint8)
    x = 3
    for d in range(168, 185):
        if x + 2 * d + 2 >= W:
            break
        occ[:, x] = 1
        x += 2 * d + 1
    occ[:, min(x, W - 1)] = 1
    occ2 = np.zeros((H, W), np.uint8)
    occ2[0, :] = 1; occ2[H - 1, ::3] = 1          # vertical distances up to 209 in the middle rows
    d2 = ctx.edt(torch.from_numpy(np.stack([occ, occ2])).cuda())
    torch.cuda.synchronize()
    got = d2.cpu().numpy()
    assert np.array_equal(got[0], oracle.edt(occ))
    assert np.array_equal(got[1], oracle.edt(occ2))


def test_edt_wide_many_groups_per_workgroup(ctx, oracle):
    """More row groups than workgroups (the persistent kernel's slots are reused many times): 3 grids of 2048 x 1500 are
    282 groups on at most 256 workgroups -- and 36 grids of 1040 x 200 give every workgroup several -- against the oracle."""
    import torch
    from sea_current_amd import synth
    occ = np.stack([synth.block_grid(2048, 1500, 0.2, seed=70 + i) for i in range(3)])
    got = ctx.edt(torch.from_numpy(occ).cuda()).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], oracle.edt(occ[i])), i
    occ = np.stack([synth.salt_grid(1040, 200, 0.02 * (1 + i % 5), seed=90 + i) for i in range(36)])
    got = ctx.edt(torch.from_numpy(occ).cuda()).cpu().numpy()
    for i in range(36):
        assert np.array_equal(got[i], oracle.edt(occ[i])), i


def test_two_contexts_two_threads_big_lds_kernels(oracle):
    """Two contexts driven from two host threads at once through the kernels that need more than 64 KiB of dynamic LDS
    (4096-wide rows: the whole-row kernel with its 128 KiB of distance bytes): the raised LDS limit is per context, so
    neither depends on the other having run first."""
    import threading
    import torch
    import sea_current_amd as sc
    from sea_current_amd import synth
    occs = [synth.block_grid(4096, 96, 0.2, seed=41), synth.salt_grid(4096, 96, 0.2, seed=42)]
    refs = [oracle.edt(o) for o in occs]
    res, errs = [None, None], []

    def work(i):
        try:
            c = sc.Context(0, use_torch_stream=False)
            d2 = c.edt(torch.from_numpy(occs[i]).cuda())
            tp = None
            if i == 0:   # TOPP-RA's kernel raises its limit too
                pl = synth.toppra_plans(4, dof=16)
                t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
                tp = c.toppra(t(pl["p0"]), t(pl["p1"]), t(pl["v0"]), t(pl["v1"]), t(-pl["vlim"]), t(pl["vlim"]), t(-pl["alim"]), t(pl["alim"]), N=200)
            c.synchronize()
            res[i] = d2.cpu().numpy()
            assert tp is None or int((tp["status"] >= 0).sum()) == 4
            c.close()
        except Exception as e:  # surfaced below
            errs.append(e)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert np.array_equal(res[i], refs[i]), i


@pytest.mark.parametrize("W", [1100, 2048, 3000, 4096])
def test_edt_wide_open_space(ctx, oracle, W):
    """Rows the packed cascade cannot settle (distances beyond 175 columns) go through the site search: the columns with an
    obstacle, compacted, and the monotone nearest-site rule.  Cases: a handful of obstacles (few sites), a dense half beside
    an empty half (more sites than one pass holds: several passes), obstacles only in the last / first columns, one full
    column, and a tall sparse grid whose vertical distances exceed a band by far."""
    import torch
    rng = np.random.default_rng(W + 1)
    H = 96
    few = np.zeros((H, W), np.uint8)
    for _ in range(9):
        few[rng.integers(0, H), rng.integers(0, W)] = 1
    half = np.zeros((H, W), np.uint8)
    half[:, :W // 2] = (rng.random((H, W // 2)) < 0.3)
    half[:, W // 2 + 40:] = 0
    ends = np.zeros((H, W), np.uint8); ends[5, W - 1] = 1; ends[H - 2, 0] = 1
    col = np.zeros((H, W), np.uint8); col[:, W // 3] = 1
    dense_left = np.zeros((H, W), np.uint8); dense_left[::2, :W - 400] = 1      # every column a site for most of the row, open space at its end
    occ = np.stack([few, half, ends, col, dense_left])
    got = ctx.edt(torch.from_numpy(occ).cuda()).cpu().numpy()
    for b in range(occ.shape[0]):
        assert np.array_equal(got[b], oracle.edt(occ[b])), b
    tall = (rng.random((1500, W)) < 3e-5).astype(np.uint8)
    tall[0, 0] = 1
    assert np.array_equal(ctx.edt(torch.from_numpy(tall).cuda()).cpu().numpy(), oracle.edt(tall))


def test_edt_open_space_mode_up_to_1024_columns(oracle):
    """Rows of 513 .. 1024 pixels: a context that has met open space (rows the packed cascade cannot settle) runs the band
    kernel's build with the site search from its next synchronisation on, and goes back once a launch finds none.  Results
    are the oracle's in every state: first call (32-bit fallback), adapted calls (site search), mixed batches, and back."""
    import torch
    import sea_current_amd as sc
    c = sc.Context(0)
    rng = np.random.default_rng(77)
    for W, H in ((1024, 300), (700, 200), (1000, 1100)):
        sparse = np.stack([(rng.random((H, W)) < p).astype(np.uint8) for p in (2e-5, 1e-4, 4e-4)])
        sparse[0, H // 2, W // 3] = 1
        dense = np.stack([(rng.random((H, W)) < 0.2).astype(np.uint8), np.zeros((H, W), np.uint8), sparse[1]])
        one_col = np.zeros((1, H, W), np.uint8); one_col[0, :, W - 3] = 1
        refs = {id(a): [oracle.edt(g) for g in a] for a in (sparse, dense, one_col)}
        for a in (sparse, sparse, sparse, dense, dense, one_col, sparse, dense, dense, dense):
            got = c.edt(torch.from_numpy(a).cuda())
            c.synchronize()
            got = got.cpu().numpy()
            for k in range(a.shape[0]):
                assert np.array_equal(got[k], refs[id(a)][k]), (W, H, k)
    c.close()


@pytest.mark.parametrize("W", [1024, 600])
def test_edt_open_space_mode_is_per_context(oracle, W):
    """Two contexts on one device: the open-space hint of edt_band_k16_kernel belongs to the context that launched it.  A (a
    map of open space) enters open mode at its synchronisation, whichever context synchronises first, and reserves the
    up / down words at its next call; B (a dense map) reserves nothing."""
    import torch
    import sea_current_amd as sc
    H, batch = 64, 1
    rng = np.random.default_rng(W)
    occ_a = np.zeros((H, W), np.uint8); occ_a[32, 10] = 1      # every row has distances beyond 175 columns: the fallback
    occ_b = (rng.random((H, W)) < 0.2).astype(np.uint8)
    ref_a, ref_b = oracle.edt(occ_a), oracle.edt(occ_b)
    ta, tb = torch.from_numpy(occ_a).cuda(), torch.from_numpy(occ_b).cuda()
    A, B = sc.Context(0), sc.Context(0)
    try:
        got = [(A.edt(ta), ref_a), (B.edt(tb), ref_b)]
        torch.cuda.synchronize()
        B.synchronize(); A.synchronize()
        a1, b1 = A.scratch_bytes(), B.scratch_bytes()
        got += [(A.edt(ta), ref_a), (B.edt(tb), ref_b)]
        torch.cuda.synchronize()
        B.synchronize(); A.synchronize()
        a2, b2 = A.scratch_bytes(), B.scratch_bytes()
    finally:
        A.close(); B.close()
    for d, ref in got:
        assert np.array_equal(d.cpu().numpy(), ref)
    assert b2 == b1, "B never met open space: no up / down words"
    assert a2 == a1 + batch * ((H + 31) // 32) * W * 4, "A met open space: its next call runs the OPEN build"
