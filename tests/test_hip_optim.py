"""dtc_sgd_step, ClippedSGD and fast_rcnn_train_step on the MI355X (-m gpu).  p and buf are compared BIT FOR BIT with the numpy
restatement (tests/optim_ref.py), which is fed the clip factor the test recomputes in float32 from the reported total_norm;
stats[1] must be that recomputation bit for bit and stats[0] lie within one float32 ulp of the float64 norm.  Every p and buf is
followed by 64 guard words of 0xFF, the workspace and stats start as 0xFF, and g must come back unchanged.  A NaN equals a NaN
whatever its payload (IEEE 754 leaves the payload of an invalid operation open; numpy on the host and the GPU choose differently).
tests/README_optim.md has the table of cases."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as orf
from detectorch_amd import synth

pytestmark = pytest.mark.gpu

GUARD = 64
TINY = float(np.finfo(np.float32).tiny)
HYPER = [(0.05, 1e-4), (0.01, 0.0)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """equal bit patterns, a NaN matching any NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _guarded(values, phase):
    """values on the device `phase` elements past a 16-byte boundary, 64 guard words of 0xFF behind -> (view, whole allocation)"""
    n = values.size
    whole = torch.full((phase + n + GUARD,), -1, dtype=torch.int32, device="cuda").view(torch.float32)     # 0xFFFFFFFF
    view = whole[phase:phase + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32)))
    assert view.data_ptr() % 16 == 4 * phase
    return view, whole


def _guards_intact(whole, phase, n):
    w = whole.view(torch.int32).cpu().numpy()
    return bool(np.all(w[:phase] == -1) and np.all(w[phase + n:] == -1))


class Run:
    """One set of tensors on the device with its plan; step() makes one dtc_sgd_step and checks it against the restatement."""

    def __init__(self, p, g, buf=None, groups=None, hyper=HYPER, phases=None):
        from detectorch_amd import hip_optim
        self.ho = hip_optim
        n = len(p)
        self.p = [np.array(a, np.float32).ravel() for a in p]
        self.g = [np.array(a, np.float32).ravel() for a in g]
        self.buf = [np.zeros_like(a) if buf is None else np.array(buf[k], np.float32).ravel() for k, a in enumerate(self.p)]
        self.groups = list(groups) if groups is not None else [0] * n
        self.hyper = [tuple(h) for h in hyper]
        self.phases = phases if phases is not None else [(0, 0, 0)] * n
        self.dp, self.dg, self.db = ([_guarded(a[k], self.phases[k][j]) for k in range(n)] for j, a in enumerate((self.p, self.g, self.buf)))
        self.plan = hip_optim.make_plan([v for v, _ in self.dp], [v for v, _ in self.dg], [v for v, _ in self.db], self.groups,
                                        len(self.hyper))
        assert self.plan.n_chunks == len(orf.chunk_table([a.size for a in self.p]))
        self.plan.workspace.fill_(0xFF)
        self.dhyper = torch.tensor(self.hyper, dtype=torch.float32, device="cuda")
        self.stats = torch.full((4,), -1, dtype=torch.int32, device="cuda").view(torch.float32)

    def step(self, momentum=0.9, max_norm=35.0, skip_nonfinite=False):
        """-> (total_norm, coef, nonfinite) as reported, after the checks every case shares"""
        self.ho.sgd_step(self.plan, self.dhyper, momentum, max_norm, self.stats, skip_nonfinite)
        torch.cuda.synchronize()
        total, coef, nonfinite, zero = self.stats.cpu().numpy()
        with np.errstate(over="ignore"):
            want_norm = orf.norm64(self.g)
            finite = bool(np.isfinite(np.float32(want_norm)))
        print("total_norm %r (float64 %r) coef %r nonfinite %r" % (total, want_norm, coef, nonfinite))
        if finite:
            assert abs(float(total) - want_norm) <= float(np.spacing(np.float32(want_norm)))      # one float32 ulp
        else:
            assert np.isnan(total) if np.isnan(want_norm) else total == np.inf                     # 6e38 rounds to inf
        want_coef = orf.coef32(total, max_norm)
        assert same(coef, want_coef), (coef, want_coef)
        assert nonfinite == (0.0 if np.isfinite(total) else 1.0) and bits(zero) == 0
        if not (skip_nonfinite and nonfinite):
            orf.step32(self.p, self.g, self.buf, want_coef, self.hyper, self.groups, momentum)
        for k in range(len(self.p)):
            n = self.p[k].size
            assert same(self.dp[k][0].cpu().numpy(), self.p[k]), ("p", k)
            assert same(self.db[k][0].cpu().numpy(), self.buf[k]), ("buf", k)
            assert np.array_equal(bits(self.dg[k][0].cpu().numpy()), bits(self.g[k])), ("g", k)    # never written
            for j, d in enumerate((self.dp, self.dg, self.db)):
                assert _guards_intact(d[k][1], self.phases[k][j], n), ("guard", k, j)
        return total, coef, nonfinite


def _data(rs, sizes, scale=1.0):
    return [(rs.standard_normal(n) * scale).astype(np.float32) for n in sizes]


def _chunk():
    from detectorch_amd import hip_optim
    return hip_optim.CHUNK


# ---- (a), (b): one tensor; the vector body with head and tail, the block edge, the chunk edge ---------------------------------------
EDGE_SIZES = ["1", "3", "4", "5", "255", "256", "257", "1023", "1024", "1025", "CHUNK-1", "CHUNK", "CHUNK+1", "2*CHUNK+1"]


@pytest.mark.parametrize("size", EDGE_SIZES)
def test_one_tensor(size):
    n = eval(size, {"CHUNK": _chunk()})
    rs = synth.rng(70, n)
    r = Run(_data(rs, [n]), _data(rs, [n]), _data(rs, [n], 0.1))
    assert r.plan.n_chunks == -(-n // _chunk())
    r.step()
    r.step()


# ---- (c): the table, the per-group hyper-parameters, the fixed-order norm over many chunks -------------------------------------------
def test_many_tensors_two_groups():
    rs = synth.rng(71, 0)
    sizes = [1, 5000] + [int(v) for v in rs.randint(1, 5001, 35)] + [3 * _chunk() + 7]
    assert len(sizes) == 38
    groups = [k % 2 for k in range(38)]
    p0, g0, b0 = _data(rs, sizes), _data(rs, sizes, 0.2), _data(rs, sizes, 0.1)
    r = Run(p0, g0, b0, groups)
    assert r.plan.n_chunks >= 38 + 3
    total, coef, _ = r.step()
    assert coef < 1.0                                                                       # clipped: every element sees the norm
    # the groups' hyper-parameters reached their tensors: with the rows swapped every tensor differs
    s = Run(p0, g0, b0, groups, hyper=HYPER[::-1])
    s.step()
    assert not any(same(a, b) for a, b in zip(r.p[1:], s.p[1:]))


# ---- (d): the dword path and its choice per chunk ------------------------------------------------------------------------------------
def test_every_misalignment_in_one_call():
    rs = synth.rng(72, 0)
    phases = [(a, b, c) for a in range(4) for b in range(4) for c in range(4)]
    sizes = [1031] * 64
    r = Run(_data(rs, sizes), _data(rs, sizes), _data(rs, sizes, 0.1), [k % 2 for k in range(64)], phases=phases)
    assert r.plan.n_tensors == r.plan.n_chunks == 64
    r.step()
    r.step(momentum=0.5, max_norm=3.0)


# ---- (e): the clip --------------------------------------------------------------------------------------------------------------------
def test_clip_engaged_or_not():
    rs = synth.rng(73, 0)
    sizes = [300, 4097, 17]
    p, g = _data(rs, sizes), _data(rs, sizes, 0.1)
    total, coef, _ = Run(p, g).step()
    assert total < 35.0 and bits(coef) == bits(np.float32(1.0))
    # coef exactly 1: the result does not depend on the norm's bits -- the same step with max_norm far away gives the same bits
    a, b = Run(p, g), Run(p, g)
    a.step(max_norm=35.0)
    b.step(max_norm=1e30)
    assert all(same(x, y) for x, y in zip(a.p, b.p)) and all(same(x, y) for x, y in zip(a.buf, b.buf))
    total, coef, _ = Run(p, [v * np.float32(1e4) for v in g]).step()
    assert total > 3500.0 and 0.0 < coef < 0.01
    total, coef, _ = Run([np.float32([0.5])], [np.float32([35.0])]).step(max_norm=35.0)
    assert total == 35.0 and np.float32(35.0) + np.float32(1e-6) == np.float32(35.0) and bits(coef) == bits(np.float32(1.0))
    total, coef, nonfinite = Run(p, [v * np.float32(1e4) for v in g]).step(max_norm=float("inf"))
    assert total > 3500.0 and bits(coef) == bits(np.float32(1.0)) and nonfinite == 0.0


# ---- (f): denormals, overflow of the float32 norm, NaN, inf -------------------------------------------------------------------------
def test_denormal_gradients_are_kept():
    rs = synth.rng(74, 0)
    sizes = [5, 1200]
    g = [(v * np.float32(1e-40)).astype(np.float32) for v in _data(rs, sizes)]
    assert all(0 < np.abs(v).max() < TINY for v in g)
    r = Run([np.zeros(n, np.float32) for n in sizes], g, hyper=[(0.5, 1e-4)])
    total, coef, nonfinite = r.step()
    assert 0.0 < total < TINY and bits(coef) == bits(np.float32(1.0)) and nonfinite == 0.0     # float32 squares would all be zero
    for p, b in zip(r.p, r.buf):
        assert 0 < np.abs(b).max() < TINY and 0 < np.abs(p).max() < TINY and np.count_nonzero(p) > p.size // 2
    r.step()                                                                                   # denormal sums: momentum * buf + d


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("kind", ["overflow", "nan", "inf"])
def test_nonfinite_norm(kind, skip):
    rs = synth.rng(75, 0)
    sizes = [4, 700, 4100]
    p, g, buf = _data(rs, sizes), _data(rs, sizes), _data(rs, sizes, 0.1)
    if kind == "overflow":
        g[0][:] = 3e38                                                                         # finite, the float32 norm is not
    else:
        g[2][4099] = np.nan if kind == "nan" else np.inf
    r = Run(p, g, buf, [0, 1, 0])
    before = [a.copy() for a in r.p + r.buf]
    total, coef, nonfinite = r.step(skip_nonfinite=skip)
    assert nonfinite == 1.0 and (np.isnan(total) if kind == "nan" else total == np.inf)
    assert np.isnan(coef) if kind == "nan" else coef == 0.0
    if skip:                                                                                   # (Run.step compared the device's bytes)
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before, r.p + r.buf))
    elif kind == "overflow":                                                                   # coef 0: weight decay and momentum alone
        assert all(np.isfinite(a).all() for a in r.p + r.buf) and not any(same(x, y) for x, y in zip(before, r.p + r.buf))
    else:                                                                                      # inf * 0, NaN * coef: as written
        assert np.isnan(r.p[2][4099]) and np.isnan(r.p[0]).all() == (kind == "nan")


# ---- (g): consecutive steps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_five_steps(momentum):
    rs = synth.rng(76, 0)
    sizes = [33, 4096, 700, 1]
    r = Run(_data(rs, sizes), _data(rs, sizes), None, [0, 1, 1, 0])
    for step in range(5):
        g = _data(rs, sizes, 30.0 if step % 2 else 0.3)                                        # clipped and not, in turn
        for k, (view, _) in enumerate(r.dg):
            view.copy_(torch.from_numpy(g[k]))
        r.g = g
        total, coef, _ = r.step(momentum=momentum)
        assert (coef < 1.0) == bool(step % 2)
    if momentum == 0.0:                                                                        # the buffer is the last update alone:
        assert same(r.buf[1], r.g[1] * coef)                                                   # group 1 has no weight decay


# ---- (h): the same bits eagerly, again, and under graph replay ------------------------------------------------------------------------
def _params(rs, sizes):
    return [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in _data(rs, sizes)]


def test_eager_repeat_and_graph_replay():
    from detectorch_amd.optim import ClippedSGD
    sizes = [257, 3 * _chunk() + 7, 1000, 3]
    g1, g2 = _data(synth.rng(77, 1), sizes, 20.0), _data(synth.rng(77, 2), sizes, 0.05)

    def make(capturable):
        params = _params(synth.rng(77, 0), sizes)
        opt = ClippedSGD([dict(params=params[:2]), dict(params=params[2:], lr=0.02, weight_decay=0.0)], lr=0.05, capturable=capturable)
        for p, g in zip(params, g1):
            p.grad = torch.from_numpy(g).cuda()
        return params, opt

    def state(params, opt):
        torch.cuda.synchronize()
        return [p.detach().cpu().numpy().copy() for p in params] + [opt.state[p]['momentum_buffer'].cpu().numpy().copy() for p in params] + \
            [opt.stats.cpu().numpy().copy()]

    (pa, oa), (pb, ob), (pc, oc) = make(False), make(False), make(True)
    oa.step(); ob.step()
    one = state(pa, oa)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(one, state(pb, ob)))           # two eager calls, equal inputs
    assert one[-1][1] < 1.0                                                                   # clipped
    oa.step()
    two = state(pa, oa)
    assert oc.prepare() and oc.stats is not None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oc.step()
    start = state(pc, oc)
    assert all(np.array_equal(bits(x.detach().cpu().numpy()), bits(y)) for x, y in zip(_params(synth.rng(77, 0), sizes), start[:4]))
    graph.replay()
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(one, state(pc, oc)))
    graph.replay()
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(two, state(pc, oc)))
    # g and lr rewritten in place: the replay gives the eager bits of the new values
    for params in (pa, pc):
        for p, g in zip(params, g2):
            p.grad.copy_(torch.from_numpy(g))
    for grp in oa.param_groups:
        grp['lr'] = 0.003
    oc.set_lr_(0.003)
    oa.step()
    graph.replay()
    three = state(pa, oa)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(three, state(pc, oc)))
    assert three[-1][1] == 1.0 and not np.array_equal(bits(three[0]), bits(two[0]))
    # zero_grad(set_to_none=True) moves the gradients: the table follows, in memory of its own
    old, keep = oa._plan.table, [p.grad for p in pa]                                          # (kept: their addresses are not reused)
    oa.zero_grad(set_to_none=True)
    for p, g in zip(pa, g1):
        p.grad = torch.from_numpy(g).cuda() * 1.0
    oa.step()
    torch.cuda.synchronize()
    assert oa._plan.table is not old and oa._plan.table.data_ptr() != old.data_ptr()


# ---- (i): bad arguments write nothing ---------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_every_byte():
    from detectorch_amd import hip, hip_optim
    n = 1000
    ff = lambda words: torch.full((words,), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    p, g, buf, stats, hyper = ff(n), ff(n), ff(n), ff(4), torch.tensor(HYPER, dtype=torch.float32, device="cuda")
    plan = hip_optim.make_plan([p], [g], [buf], [0], 2)
    plan.workspace.fill_(0xFF)
    L = hip_optim.lib()
    tb, ws = plan.table.numel(), plan.workspace.numel()
    assert (tb, ws) == (48, 16)

    def call(n_tensors=1, n_chunks=1, n_groups=2, plan_bytes=tb, momentum=0.9, max_norm=35.0, flags=0, workspace_bytes=ws, **kw):
        v = lambda k, t: None if k in kw and kw[k] is None else C.c_void_p(t.data_ptr() + kw.get(k, 0))
        return L.dtc_sgd_step(v("plan_dev", plan.table), plan_bytes, n_tensors, n_chunks, v("group_hyper_dev", hyper), n_groups,
                              momentum, max_norm, flags, v("workspace", plan.workspace), workspace_bytes, v("stats", stats),
                              hip.stream_ptr())

    cases = [(dict(plan_dev=None), -1), (dict(group_hyper_dev=None), -1), (dict(stats=None), -1), (dict(workspace=None), -3),
             (dict(max_norm=0.0), -1), (dict(max_norm=-35.0), -1), (dict(max_norm=float("nan")), -1), (dict(momentum=1.0), -1),
             (dict(momentum=-0.5), -1), (dict(momentum=float("nan")), -1), (dict(workspace_bytes=ws - 1), -3), (dict(workspace=8), -1),
             (dict(plan_dev=8), -1), (dict(stats=2), -1), (dict(group_hyper_dev=1), -1), (dict(n_tensors=0), -1),
             (dict(n_chunks=0), -1), (dict(n_groups=0), -1), (dict(n_groups=65), -4), (dict(flags=4), -1),
             (dict(plan_bytes=tb + 16), -1), (dict(n_tensors=16385, n_chunks=16385, plan_bytes=16385 * 48), -4),
             (dict(n_chunks=2050, plan_bytes=32 + 2050 * 16), -4)]
    for kw, want in cases:
        assert call(**kw) == want, kw
    torch.cuda.synchronize()
    for t in (p, g, buf, stats, plan.workspace):
        assert bool((t.view(torch.uint8) == 0xFF).all())
    assert call() == 0                                                                         # and the good call is good
    torch.cuda.synchronize()
    assert not bool((stats.view(torch.uint8) == 0xFF).all())
    with pytest.raises(TypeError):
        hip_optim.make_plan([p.double()], [g.double()], [buf.double()], [0], 1)
    with pytest.raises(TypeError):
        hip_optim.make_plan([ff(2 * n)[::2]], [g], [buf], [0], 1)


# ---- (j): against clip_grad_norm_ + torch.optim.SGD on the same GPU -------------------------------------------------------------------
def test_against_torch_sgd_on_an_mlp():
    from detectorch_amd.optim import ClippedSGD
    rs = synth.rng(78, 0)
    dims = [(40, 48), (48, 20), (20, 3)]                                                       # 1968 + 980 + 63 = 3011 parameters
    init = [a for i, o in dims for a in ((rs.standard_normal((o, i)) / np.sqrt(i)), rs.standard_normal(o) * 0.1)]
    assert sum(a.size for a in init) == 3011
    xs = [rs.standard_normal((32, 40)) * 2.0 for _ in range(10)]
    ys = [rs.standard_normal((32, 3)) * 6.0 for _ in range(10)]
    max_norm = 35.0

    def run(dtype, dev, ours):
        params = [torch.nn.Parameter(torch.tensor(a, dtype=dtype, device=dev)) for a in init]
        groups = [dict(params=params[0::2]), dict(params=params[1::2], weight_decay=0.0)]
        opt = ClippedSGD(groups, lr=0.05, max_norm=max_norm) if ours else torch.optim.SGD(groups, lr=0.05, momentum=0.9, weight_decay=1e-4)
        norms = []
        for x, y in zip(xs, ys):
            h = torch.tensor(x, dtype=dtype, device=dev)
            for k in range(3):
                h = torch.nn.functional.linear(h, params[2 * k], params[2 * k + 1])
                h = torch.relu(h) if k < 2 else h
            loss = ((h - torch.tensor(y, dtype=dtype, device=dev)) ** 2).sum() / 30.0
            opt.zero_grad()
            loss.backward()
            if ours:
                opt.step()
                norms.append(float(opt.stats[0]))
            else:
                norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
                opt.step()
        return [p.detach().double().cpu().numpy() for p in params], norms

    y64, n64 = run(torch.float64, "cpu", False)
    mine, n_mine = run(torch.float32, "cuda", True)
    theirs, n_theirs = run(torch.float32, "cuda", False)
    assert min(n64) < max_norm < max(n64)                                                      # both regimes occur
    dist = lambda got: max(float(np.max(np.abs(a - b)) / (orf.EPS32 * np.max(np.abs(b)))) for a, b in zip(got, y64))
    d_mine, d_theirs = dist(mine), dist(theirs)
    print("distance from the float64 run after 10 steps, in eps32 * max|p|: ClippedSGD %.3f, clip_grad_norm_ + SGD %.3f; norms %s"
          % (d_mine, d_theirs, ["%.2f" % v for v in n64]))
    assert d_mine <= 4.0 * d_theirs


# ---- (k): the training step ---------------------------------------------------------------------------------------------------------------
def test_fast_rcnn_train_step():
    from detectorch_amd.model.detector import detector
    from detectorch_amd.optim import ClippedSGD
    from detectorch_amd.train import fast_rcnn_train_step, freeze_stem
    from detectorch_amd.utils import fast_rcnn_sample_rois as fs
    from detectorch_amd.utils.solver import get_lr_at_iter
    torch.manual_seed(5)
    model = detector(N_classes=5).cuda()
    trainable = freeze_stem(model)
    opt = ClippedSGD(trainable, lr=0.01)
    rs = synth.rng(79, 0)
    images = torch.from_numpy(rs.standard_normal((1, 3, 64, 96)).astype(np.float32)).cuda()
    gt = np.array([[[8, 6, 60, 50], [40, 20, 90, 60]]], np.float32)
    jit = rs.uniform(-6, 6, (1, 20, 4)).astype(np.float32)
    near = np.clip(gt[:, [0, 1] * 10] + jit, 0, [95, 63, 95, 63]).astype(np.float32)
    x1, y1 = rs.uniform(0, 60, (1, 10)), rs.uniform(0, 40, (1, 10))
    far = np.stack([x1, y1, x1 + rs.uniform(8, 35, (1, 10)), y1 + rs.uniform(8, 23, (1, 10))], -1).astype(np.float32)
    d = lambda a, t=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).to("cuda", t)
    blobs = fs.sample_rois_batched(d(np.concatenate([near, far], 1)), d([30], torch.int32), d(gt), d([[1, 3]], torch.int32),
                                   d([[0, 0]], torch.int32), d([2], torch.int32), d([1.0]),
                                   rand_keys=d(rs.randint(0, 2 ** 31 - 1, (1, 32)), torch.int32), rois_per_image=16, num_classes=5,
                                   expanded=False)
    assert blobs["rois"].shape == (1, 16, 5) and int(blobs["n_fg"][0]) >= 1
    names = {id(p): n for n, p in model.named_parameters()}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    loss_cls, loss_bbox, acc = fast_rcnn_train_step(model, opt, images, blobs, it=0)
    torch.cuda.synchronize()
    print("loss_cls %r loss_bbox %r accuracy %r stats %r" % (float(loss_cls), float(loss_bbox), float(acc), opt.stats.cpu().numpy()))
    assert np.isfinite(float(loss_cls)) and np.isfinite(float(loss_bbox)) and float(loss_cls) > 0 and 0.0 <= float(acc) <= 1.0
    assert opt.param_groups[0]['lr'] == get_lr_at_iter(0) < 0.01                               # the solver's warm-up
    total, coef = opt.stats.cpu().numpy()[:2]
    assert same(coef, orf.coef32(total, 35.0)) and np.isfinite(total) and total > 0
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert frozen and all(torch.equal(before[n], dict(model.named_parameters())[n]) for n in frozen)
    assert all(p.grad is None for n, p in model.named_parameters() if not p.requires_grad)
    grads = [p.grad.cpu().numpy().ravel() for p in trainable]
    assert abs(float(total) - orf.norm64(grads)) <= float(np.spacing(np.float32(orf.norm64(grads))))
    want_p = [before[names[id(p)]].cpu().numpy().ravel().copy() for p in trainable]
    want_b = [np.zeros_like(a) for a in want_p]
    lr = np.float32(opt.param_groups[0]['lr'])
    orf.step32(want_p, grads, want_b, coef, [(lr, 1e-4)], [0] * len(trainable), 0.9)
    for p, a, b in zip(trainable, want_p, want_b):
        assert same(p.detach().cpu().numpy().ravel(), a), names[id(p)]
        assert same(opt.state[p]['momentum_buffer'].cpu().numpy().ravel(), b), names[id(p)]
    assert float(model.model.layer2[0].conv1.weight.grad.abs().max()) > 0                      # the gradient reached the body
    fast_rcnn_train_step(model, opt, images, blobs, it=1)                                      # a second step runs
    torch.cuda.synchronize()
    assert np.isfinite(opt.stats.cpu().numpy()).all() and opt.param_groups[0]['lr'] > float(lr)
    # the inference entries of the same model are what a model that never trained computes from the same weights.  Not bit for bit:
    # the convolution and GEMM libraries underneath do not repeat their own bits from call to call on one model (1e-8 on logits of
    # 0.2, measured on a model that never trained).  The bound is the reordering of the longest reduction, 3 * 3 * 512 = 4608 terms
    # of res5: a random walk of sqrt(4608) = 68 roundings of eps32, on the scale of the output.
    fresh = detector(N_classes=5).cuda()
    fresh.load_state_dict(model.state_dict())
    rois = blobs["rois"][0, :, 1:].contiguous()
    for m in (model, fresh):
        assert not m.training
        m.out = m(images, rois=rois)[:2]
        path = m.forward_batched(images, [1.0], [[64.0, 96.0]], proposals=rois[None].contiguous(), proposal_counts=[16])
        m.out_b = (path.cls_logits_out.clone(), path.bbox_pred_out.clone())
    torch.cuda.synchronize()
    assert not model.out[0].requires_grad and not model.out[1].requires_grad
    for a, b in zip(model.out + model.out_b, fresh.out + fresh.out_b):
        dist = float((a - b).abs().max()) / (orf.EPS32 * float(b.abs().max()))
        print("inference after training against a fresh model on the same weights: %.3f eps32 * max|out|" % dist)
        assert a.shape == b.shape and dist <= np.sqrt(4608.0)
    # ... and they did change with the weights
    assert not torch.equal(before["classif_head.weight"], model.classif_head.weight)
