"""GPU: the nearest-neighbour check on the device -- mcvd_knn_search, mcvd_hflip_u8 and mcvd_nn_collect (kernels/prdc.cpp) through the C
ABI -- against tests/nn_ref.py (fp64 numpy, direct differences, ties to the lower index) and what the REAL
evaluation/nearest_neighbor.py computed (tests/golden/nearest_neighbor.pt; the CPU side is tests/test_nearest_neighbor_cpu.py).

Gates:
  * indices: equal to the restatement row for row, after the precondition ON THE RESTATEMENT that the relative gap between consecutive
    entries among every row's first k + 1 sorted squared distances is at least 1e-9 (the Gaussian sets here hold 2.9e-6 and more);
  * squared distances: the bound include/mcvd_hip.h derives for the Gram form against the direct form, per pair:
    gamma_(d+3) (|a| + |b|)^2, |a| the larger norm of the two views (nn_ref.pair_bound); derived, not measured;
  * pieces, runs and the equal-d2 run of a repeated row: bit patterns, torch.equal;
  * the mirror and the collected images: exact;
  * the fixture: indices and plot_data exact, distances within 8 x the fixture's ref_rel_dev of the reference's.
Measured ratios are printed by every test; on an MI355X the squared distances reach at most 0.222 of the bound (d = 5; 0.155 at the
forced-split shape, 0.083 at d = 33, 0.001 at d = 2048), and the fixture's distances sit at most 1.000 x ref_rel_dev from the reference's."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import nn_ref, prdc_ref
from tests.test_nearest_neighbor_cpu import NAMES, distances_within, restated

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
_pool = {}


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ctx():
    from mcvd_pytorch_amd import metrics
    dev = torch.device("cuda", torch.cuda.current_device())
    return metrics._package_ctx(dev), dev


def c_search(q, r, k, q2=None, index_base=0, state=None, d=None):
    """mcvd_knn_search on device tensors as they are (any row stride): (dist2, index), a fresh pair or the merged copy of `state`."""
    from mcvd_pytorch_amd import _lib
    ctx, dev = _ctx()
    code = lambda t: _lib.F64 if t.dtype == F64 else _lib.F32      # noqa: E731
    Nq, d = len(q), (q.shape[1] if d is None else d)
    if state is None:
        dist2, index = torch.full((Nq, k), -5.0, dtype=F64, device=dev), torch.full((Nq, k), -7, dtype=torch.int64, device=dev)
    else:
        dist2, index = state[0].clone(), state[1].clone()
    rc = _lib.lib.mcvd_knn_search(ctx, P(q), code(q), q.stride(0), P(q2), code(q2) if q2 is not None else 0, q2.stride(0) if q2 is not None else 0, Nq,
                                  P(r), code(r), r.stride(0), len(r), d, k, index_base, 0 if state is None else 1, P(dist2), P(index))
    assert rc == 0, _lib.last_error()
    return dist2, index


def pool(d, n=65, seed=0):
    """Gaussian rows drawn in fp32 (the fp32 and the fp64 inputs hold the same numbers): two query views and a ref set of n rows, and the
    restated squared distances [n, n] for one view and for two."""
    if (d, n, seed) not in _pool:
        g = torch.Generator().manual_seed(100 + d + seed)
        q, q2, r = (torch.randn(n, d, generator=g) for _ in range(3))
        one = prdc_ref.dist2(q.double().numpy(), r.double().numpy())
        two = np.minimum(one, prdc_ref.dist2(q2.double().numpy(), r.double().numpy()))
        _pool[(d, n, seed)] = dict(q=q, q2=q2, r=r, one=one, two=two)
    return _pool[(d, n, seed)]


def _held_to(got, want_d2, want_i, bound, k, what):
    """Indices equal; d2 under the derived bound.  Returns the largest ratio."""
    gd, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(gi, want_i), what
    live = want_i >= 0
    assert np.array_equal(np.isinf(gd), ~live), what
    ratio = float((np.abs(gd - want_d2)[live] / bound[live]).max()) if live.any() else 0.0
    assert ratio <= 1.0, f"{what}: {ratio}"
    return ratio


@pytest.mark.parametrize("d", [5, 33, 2048])
def test_search_against_the_restatement(d):
    """Nq in {1, 10, 65} (65: two owner blocks, the second with one live column), Nr in {k, 63, 64, 65}, k in {1, 9, 16}, one view and
    two, the dtypes cycling through fp32, fp64 and mixed; d below one staged chunk (5), a ragged chunk (33) and the maximum (2048)."""
    w = pool(d)
    combos = [(F32, F32, F32), (F64, F64, F64), (F32, F64, F64), (F64, F32, F32), (F32, F32, F64)]
    dev_rows = {dt: {name: w[name].to(dt).cuda() for name in ("q", "q2", "r")} for dt in (F32, F64)}
    worst, n_calls = 0.0, 0
    for views in (1, 2):
        full = w["one"] if views == 1 else w["two"]
        for k in (1, 9, 16):
            for Nr in (k, 63, 64, 65):
                for Nq in (1, 10, 65):
                    d2 = full[:Nq, :Nr]
                    want_d2, want_i = nn_ref.search(None, None, k, d2=d2)
                    assert nn_ref.min_rel_gap(nn_ref.first_sorted(d2, k + 1)) >= 1e-9, "precondition on the inputs"
                    dq, dq2, dr = combos[n_calls % len(combos)]
                    q, r = dev_rows[dq]["q"][:Nq], dev_rows[dr]["r"][:Nr]
                    q2 = dev_rows[dq2]["q2"][:Nq] if views == 2 else None
                    bound = nn_ref.pair_bound(w["q"][:Nq].numpy(), w["r"][:Nr].numpy(), want_i, d, w["q2"][:Nq].numpy() if views == 2 else None)
                    worst = max(worst, _held_to(c_search(q, r, k, q2), want_d2, want_i, bound, k, (views, k, Nr, Nq)))
                    n_calls += 1
    print(f"  d = {d}: {n_calls} calls, squared distances at most {worst:.4f} of the bound")


def test_search_forced_split_shape():
    """d = 8, 4099 x 4099 rows: the split rule gives 8 splits of the ref axis (9 tiles each, the last 2) over 65 owner blocks; the last
    tile and the last block hold three rows.  And 65 queries against 4099 rows: 65 splits of one tile."""
    assert prdc_ref.split_plan(4099, 4099) == (65, 65, 9, 8) and prdc_ref.split_plan(4099, 65) == (2, 65, 1, 65)
    w = pool(8, n=4099)
    k = 9
    q, q2, r = (w[name].cuda() for name in ("q", "q2", "r"))
    want_d2, want_i = nn_ref.search(None, None, k, d2=w["two"])
    assert nn_ref.min_rel_gap(nn_ref.first_sorted(w["two"], k + 1)) >= 1e-9
    bound = nn_ref.pair_bound(w["q"].numpy(), w["r"].numpy(), want_i, 8, w["q2"].numpy())
    ratio = _held_to(c_search(q, r, k, q2), want_d2, want_i, bound, k, "4099 x 4099")
    ratio = max(ratio, _held_to(c_search(q[:65], r, k, q2[:65]), want_d2[:65], want_i[:65], bound[:65], k, "65 x 4099"))
    print(f"  forced split: squared distances at most {ratio:.4f} of the bound")


def test_search_all_dtypes_and_wide_rows():
    """Every dtype combination of (query, query2, ref) at one shape, and rows that are a column slice of a wider matrix (ld > d, read in
    place): the same bits as the contiguous fp64 call for fp64 rows, the same indices throughout."""
    d, k = 33, 9
    w = pool(d)
    want_d2, want_i = nn_ref.search(None, None, k, d2=w["two"])
    bound = nn_ref.pair_bound(w["q"].numpy(), w["r"].numpy(), want_i, d, w["q2"].numpy())
    base = c_search(w["q"].double().cuda(), w["r"].double().cuda(), k, w["q2"].double().cuda())
    for dq in (F32, F64):
        for dq2 in (F32, F64):
            for dr in (F32, F64):
                got = c_search(w["q"].to(dq).cuda(), w["r"].to(dr).cuda(), k, w["q2"].to(dq2).cuda())
                _held_to(got, want_d2, want_i, bound, k, (dq, dq2, dr))
                assert torch.equal(got[0], base[0]), "fp32 rows hold the same numbers: the same bits"
    for dt in (F32, F64):
        wide = lambda x, a, b: torch.cat([torch.full((len(x), a), 9.0), x, torch.full((len(x), b), -7.0)], 1).to(dt).cuda()      # noqa: E731
        q, q2, r = wide(w["q"], 2, 4)[:, 2:2 + d], wide(w["q2"], 0, 3)[:, :d], wide(w["r"], 5, 0)[:, 5:]
        assert not q.is_contiguous() and q.stride(0) == d + 6 and r.stride(0) == d + 5
        got = c_search(q, r, k, q2)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])


def test_tie_rule():
    """One ref row repeated k + 2 times at scattered positions (several tiles and splits): the copies' d2 are equal bit for bit -- the
    per-pair arithmetic does not depend on the position -- and the run comes back lowest index first."""
    d, k, Nr = 33, 9, 200
    w = pool(d, n=Nr, seed=5)
    at = [3, 17, 63, 64, 65, 100, 127, 128, 150, 190, 199]
    assert len(at) == k + 2
    r = w["r"].clone()
    r[at] = r[3].clone()
    q, q2 = w["q"][:10].clone(), w["q2"][:10].clone()
    q[0] = r[3] + 0.01 * q[0]                                  # the copies are query 0's nearest rows through the first view
    q2[1] = r[3] + 0.01 * q2[1]                                # and query 1's through the second
    want_d2, want_i = nn_ref.search(q.double().numpy(), r.double().numpy(), k, q2.double().numpy())
    assert want_i[0].tolist() == at[:k] and want_i[1].tolist() == at[:k]
    for dt in (F32, F64):
        gd, gi = c_search(q.to(dt).cuda(), r.to(dt).cuda(), k, q2.to(dt).cuda())
        assert gi[0].tolist() == at[:k] and gi[1].tolist() == at[:k], "lowest index first"
        assert bool((gd[:2] == gd[:2, :1]).all()), "the copies' d2 differ in their bits"
        assert np.array_equal(gi.cpu().numpy(), want_i), "every row, ties included"
    # k + 2 copies, k = 16 slots over the whole set of one tile
    gd, gi = c_search(q.cuda(), r[:64].cuda(), 16, q2.cuda())
    assert gi[0, :3].tolist() == [3, 17, 63] and bool((gd[0, :3] == gd[0, 0]).all()) and bool(gd[0, 3] > gd[0, 0])


def test_pieces():
    """Three unequal pieces -- one smaller than k, one of a single row -- with an index_base above 2^31: the indices and the bit pattern
    of the distances of the single call; the -1 / +inf tail after the first piece; two runs; other splits of the same set."""
    d, k, Nr, base = 33, 9, 300, (1 << 31) + 7
    w = pool(d, n=Nr, seed=1)
    q, q2, r = w["q"][:10].cuda(), w["q2"][:10].cuda(), w["r"].cuda()
    want_d2, want_i = nn_ref.search(None, None, k, d2=w["two"][:10], index_base=base)
    whole = c_search(q, r, k, q2, index_base=base)
    assert np.array_equal(whole[1].cpu().numpy(), want_i) and int(whole[1].min()) > (1 << 31)
    again = c_search(q, r, k, q2, index_base=base)
    assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1]), "two runs"
    for sizes in ([5, 1, 294], [1, 8, 291], [64, 64, 64, 64, 44], [299, 1]):
        state, at = None, 0
        for n in sizes:
            state = c_search(q, r[at:at + n], k, q2, index_base=base + at, state=state)
            if at == 0 and n < k:
                assert bool((state[1][:, n:] == -1).all()) and bool(torch.isinf(state[0][:, n:]).all()) and bool((state[1][:, :n] >= base).all())
                first_d2, first_i = nn_ref.search(None, None, k, d2=w["two"][:10, :n], index_base=base)
                assert np.array_equal(state[1].cpu().numpy(), first_i)
            at += n
        assert at == Nr
        assert torch.equal(state[1], whole[1]), sizes
        assert torch.equal(state[0], whole[0]), f"{sizes}: the distances of the pieces are not the single call's bits"


@pytest.mark.parametrize("Cc", [1, 3])
@pytest.mark.parametrize("W", [7, 8, 64])
def test_mirror(Cc, W):
    """Values at j / 255, just below them, 1.0, and outside [0, 1] (clamped): exact against the restatement."""
    from mcvd_pytorch_amd import _lib
    ctx, dev = _ctx()
    j = np.arange(256, dtype=np.float32) / np.float32(255.0)
    vals = np.concatenate([j, np.nextafter(j, np.float32(-1.0)), np.nextafter(j, np.float32(2.0)), np.array([1.0, 0.5, 2.0, -1.0, 1.0000001], dtype=np.float32)])
    n = 4
    H = -(-len(vals) // (n * Cc * W))                          # every value at least once
    x = np.resize(vals, n * Cc * H * W).reshape(n, Cc, H, W).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    out = torch.full_like(xd, -3.0)
    assert _lib.lib.mcvd_hflip_u8(ctx, P(xd), P(out), n, Cc, H, W) == 0, _lib.last_error()
    want = nn_ref.hflip_u8(x)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(np.round(out.cpu().numpy() * 255)[..., ::-1], np.clip(x * np.float32(255), 0, 255).astype(np.uint8).astype(np.float32))


def test_mirror_every_value():
    """All 256 levels, the level below each and the level above, in one [1, 1, 12, 64] image."""
    from mcvd_pytorch_amd.metrics import hflip_u8
    j = np.arange(256, dtype=np.float32) / np.float32(255.0)
    x = np.concatenate([j, np.nextafter(j, np.float32(-1.0)), np.nextafter(j, np.float32(2.0))]).reshape(1, 1, 12, 64)
    assert np.array_equal(hflip_u8(torch.from_numpy(x).cuda()).cpu().numpy(), nn_ref.hflip_u8(x))


def test_collect():
    """Three pieces through knn_search and nn_collect: after each the held images equal a gather from the concatenated set.  The second
    piece holds one row nearer to every query than all before it -- every held slot moves one place --, the third only distant rows --
    none moves."""
    from mcvd_pytorch_amd.metrics import knn_search, nn_collect
    g = torch.Generator().manual_seed(11)
    Nq, k, d = 5, 4, 6
    q = 0.01 * torch.randn(Nq, d, generator=g)
    feats = [1.0 + torch.rand(6, d, generator=g), torch.cat([torch.zeros(1, d), 5.0 + torch.rand(2, d, generator=g)]), 9.0 + torch.rand(5, d, generator=g)]
    images = [torch.rand(len(f), 3, 7, 9, generator=g) for f in feats]
    data = torch.cat(images)
    state, held, at, want = None, None, 0, None
    for step, (f, x) in enumerate(zip(feats, images)):
        old = want
        want = nn_ref.search(q.double().numpy(), f.double().numpy(), k, None, at, want)
        new = knn_search(q.cuda(), f.cuda(), k, index_base=at, state=state)
        assert np.array_equal(new[1].cpu().numpy(), want[1])
        held = nn_collect(held, None if state is None else state[1], new[1], x.cuda(), at)
        assert torch.equal(held.cpu(), data[torch.from_numpy(want[1])]), f"step {step}"
        if step == 1:
            assert (want[1][:, 0] == 6).all() and np.array_equal(want[1][:, 1:], old[1][:, :-1]), "every slot moves"
        if step == 2:
            assert np.array_equal(want[1], old[1]), "no slot moves"
        state, at = new, at + len(f)
    # a first piece smaller than k: the empty slots are zeros
    new = knn_search(q.cuda(), feats[0][:2].cuda(), k)
    held = nn_collect(None, None, new[1], images[0][:2].cuda(), 0)
    assert bool((new[1][:, 2:] == -1).all()) and bool((held[:, 2:] == 0).all()) and torch.equal(held[:, :2].cpu(), images[0][:2][new[1][:, :2].cpu()])


@pytest.mark.parametrize("name", NAMES)
def test_fixture_end_to_end(golden_dir, name):
    """NearestNeighbors on the device with the table detector evaluated on the GPU, the data set in batches of 128 and in one piece."""
    from mcvd_pytorch_amd import NearestNeighbors, nearest_neighbors
    w = restated(golden_dir, name)
    g = w["golden"]
    det = nn_ref.TableDetector(w["table"]).cuda().eval()
    batches = [(w["data"][i:i + 128].cuda(), None) for i in range(0, w["N"], 128)]
    out = nearest_neighbors(w["samples"], batches, det, k=w["k"], n_samples=w["n"])
    assert out["indices"].is_cuda and torch.equal(out["indices"].cpu(), g["indices"])
    plot = out["plot_data"].cpu()
    rows = torch.arange(len(plot)) % (w["k"] + 1) == 0
    assert torch.equal(plot[rows], w["samples"][:w["n"]]), "the sample rows"
    assert torch.equal(plot[~rows], g["plot_data"][~rows]), "the neighbour rows are copies"
    assert torch.equal(plot, g["plot_data"])
    dist = out["distances"].cpu().numpy()
    ref = g["distances"].double().numpy()
    print(f"  {name}: distances at most {(np.abs(dist - ref) / ref).max() / g['ref_rel_dev']:.3f} x ref_rel_dev {g['ref_rel_dev']:.3e}")
    assert distances_within(dist, g)
    one = NearestNeighbors(w["samples"], det, k=w["k"], n_samples=w["n"])
    one.update(w["data"])
    res = one.result()
    assert torch.equal(res["indices"], out["indices"]) and torch.equal(res["distances"], out["distances"]), "one piece: the same bits"
    assert torch.equal(res["neighbors"], out["neighbors"])


def test_every_refusal():
    """Each MCVD_EINVAL case of the three entries: code -1 with a message, and nothing launched -- the outputs keep their sentinel."""
    from mcvd_pytorch_amd import _lib, metrics
    ctx, dev = _ctx()
    x = torch.rand(8, 6, device=dev)
    d2 = torch.full((8, 3), -5.0, dtype=F64, device=dev)
    idx = torch.full((8, 3), -7, dtype=torch.int64, device=dev)
    img = torch.rand(4, 2, 3, 5, device=dev)
    flipped = torch.full_like(img, -3.0)
    held = torch.full((8, 3, 2, 3, 5), -3.0, device=dev)
    out = torch.full((8, 3, 2, 3, 5), -3.0, device=dev)
    new = torch.zeros((8, 3), dtype=torch.int64, device=dev)

    def search(q=x, qd=_lib.F32, ldq=6, q2=x, q2d=_lib.F32, ldq2=6, Nq=8, r=x, rd=_lib.F32, ldr=6, Nr=8, d=6, k=3, base=0, merge=0, o=d2, i=idx, ctx=ctx):
        return _lib.lib.mcvd_knn_search(ctx, P(q), qd, ldq, P(q2), q2d, ldq2, Nq, P(r), rd, ldr, Nr, d, k, base, merge, P(o), P(i))

    def flip(a=img, o=flipped, n=4, Cc=2, H=3, W=5, ctx=ctx):
        return _lib.lib.mcvd_hflip_u8(ctx, P(a), P(o), n, Cc, H, W)

    def collect(h=held, hi=idx, ni=new, piece=img, n=4, base=0, Nq=8, k=3, Cc=2, H=3, W=5, o=out, ctx=ctx):
        return _lib.lib.mcvd_nn_collect(ctx, P(h), P(hi), P(ni), P(piece), n, base, Nq, k, Cc, H, W, P(o))
    bad = [("k = 0", lambda: search(k=0)), ("k = 17", lambda: search(k=17)), ("d = 0", lambda: search(d=0)),
           ("d = 2049", lambda: search(d=2049, ldq=2049, ldq2=2049, ldr=2049)), ("ldq < d", lambda: search(ldq=5)), ("ldq2 < d", lambda: search(ldq2=5)),
           ("ldr < d", lambda: search(ldr=5)), ("Nq = 0", lambda: search(Nq=0)), ("Nr = 0", lambda: search(Nr=0)), ("Nq = 2^24", lambda: search(Nq=1 << 24)),
           ("Nr = 2^24", lambda: search(Nr=1 << 24)), ("q dtype", lambda: search(qd=2)), ("q2 dtype", lambda: search(q2d=-1)), ("r dtype", lambda: search(rd=3)),
           ("NULL query", lambda: search(q=None)), ("NULL ref", lambda: search(r=None)), ("NULL dist2", lambda: search(o=None)),
           ("NULL index", lambda: search(i=None)), ("NULL ctx", lambda: search(ctx=None)),
           ("flip n = 0", lambda: flip(n=0)), ("flip C = 0", lambda: flip(Cc=0)), ("flip W = 0", lambda: flip(W=0)), ("flip NULL in", lambda: flip(a=None)),
           ("flip NULL out", lambda: flip(o=None)), ("flip in place", lambda: flip(o=img)), ("flip NULL ctx", lambda: flip(ctx=None)),
           ("collect aliases held", lambda: collect(o=held)), ("collect overlaps held", lambda: collect(o=held.reshape(-1)[30:])),
           ("collect aliases the piece", lambda: collect(o=img)), ("collect k = 0", lambda: collect(k=0)),
           ("collect k = 17", lambda: collect(k=17)), ("collect Nq = 0", lambda: collect(Nq=0)), ("collect n = 0", lambda: collect(n=0)),
           ("collect C = 0", lambda: collect(Cc=0)), ("collect held without indices", lambda: collect(hi=None)),
           ("collect indices without held", lambda: collect(h=None)), ("collect NULL new", lambda: collect(ni=None)),
           ("collect NULL piece", lambda: collect(piece=None)), ("collect NULL out", lambda: collect(o=None)), ("collect NULL ctx", lambda: collect(ctx=None))]
    for name, call in bad:
        assert call() == -1, name
        assert _lib.last_error(), name
    torch.cuda.synchronize()
    assert bool((d2 == -5.0).all()) and bool((idx == -7).all()) and bool((flipped == -3.0).all()) and bool((out == -3.0).all()) \
        and bool((held == -3.0).all()), "a refused call wrote its output"
    assert search() == 0 and search(q2=None, q2d=99, ldq2=0) == 0 and flip() == 0 and collect() == 0 and collect(h=None, hi=None) == 0
    torch.cuda.synchronize()
    assert bool((d2 >= 0).all()) and bool((idx >= 0).all()) and bool((flipped >= 0).all())
    with pytest.raises(RuntimeError, match=r"code -1"):
        metrics.knn_search(x, x, k=17)
    with pytest.raises(ValueError, match="features"):
        metrics.knn_search(x[:, :5], x)
    with pytest.raises(ValueError, match="second view"):
        metrics.knn_search(x, x, k=3, query2=x[:4])
    with pytest.raises(ValueError, match="state of shapes"):
        metrics.knn_search(x, x, k=3, state=(d2[:, :2], idx[:, :2]))
