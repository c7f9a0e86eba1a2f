"""The optimizer tail without a GPU:
  * utils.solver against the reference's own values (tests/golden/solver_lr.npz, made by tests/golden/make_solver_golden.py from the
    reference's unmodified lib/utils/solver.py), compared with ==;
  * libdetectorch_optim_hip.so exports exactly what include/detectorch_optim_hip.h declares, hip_optim binds all of it under the
    header's parameter names in the header's order, and the other four libraries' export lists are the pinned ones;
  * dtc_sgd_plan, dtc_sgd_plan_bytes, dtc_sgd_workspace_bytes and the argument checks of dtc_sgd_step (validation precedes every
    HIP call) from a child process that sees no device: every return code in the stated order, nothing written on an error, the
    chunk table against its Python restatement, the sizes monotone;
  * the numpy restatement (tests/optim_ref.py) pinned to torch itself: clip_grad_norm_ + torch.optim.SGD on the CPU in float64
    against the float64 yardstick;
  * ClippedSGD's state_dict round-trips with torch.optim.SGD; step() and forward_train raise on CPU tensors.
Run as a script with --child the module prints the child's findings as JSON."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden
import optim_ref as orf

sys.path.insert(0, GOLDEN)

HEADER = os.path.join(ROOT, "include", "detectorch_optim_hip.h")
NAMES = ["dtc_optim_target_arch", "dtc_sgd_plan", "dtc_sgd_plan_bytes", "dtc_sgd_step", "dtc_sgd_workspace_bytes"]


# ---- the solver ---------------------------------------------------------------------------------------------------------------------
def test_solver_equals_the_reference_values():
    from detectorch_amd.utils import solver
    g = golden("solver_lr")
    iters = [int(i) for i in g["iters"]]
    assert iters == [0, 1, 249, 250, 499, 500, 501, 239999, 240000, 240001, 319999, 320000, 359999, 360000, 400000]
    for k, it in enumerate(iters):
        assert solver.get_step_index(it) == int(g["step_index"][k]), it
        assert solver.get_lr_at_iter(it) == float(g["lr_linear"][k]), it                             # ==: the same Python float
        assert solver.get_lr_at_iter(it, warm_up_method='constant') == float(g["lr_constant"][k]), it
        assert solver.lr_func_steps_with_decay(it) == 0.01 * 0.1 ** int(g["step_index"][k])
    assert str(g["unknown_method_error"]) == "KeyError"
    with pytest.raises(KeyError):
        solver.get_lr_at_iter(0, warm_up_method='cosine')
    assert solver.get_lr_at_iter(500, warm_up_method='cosine') == float(g["unknown_method_late"])
    # the fixture is not flat: the warm-up rises, the steps fall
    assert g["lr_linear"][0] < g["lr_linear"][2] < g["lr_linear"][5] and g["lr_linear"][8] < g["lr_linear"][7]

    class Opt:
        param_groups = [dict(lr=1.0), dict(lr=2.0)]
    solver.adjust_learning_rate(Opt, 0.25)
    assert [grp['lr'] for grp in Opt.param_groups] == [0.25, 0.25]


# ---- the library: exports and binding -----------------------------------------------------------------------------------------------
def _declared():
    """[(entry, [parameter names])] of include/detectorch_optim_hip.h, in its order"""
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = []
    for name, params in re.findall(r"\b(dtc_\w+)\s*\(([^)]*)\)\s*;", text):
        names = [] if params.strip() == "void" else [re.findall(r"\w+", p)[-1] for p in params.split(",")]
        out.append((name, names))
    return out


def test_header_symbols_are_exported_and_bound():
    from make_native_host_codes import exports
    from detectorch_amd import hip_optim
    L = hip_optim.lib()
    decl = _declared()
    assert sorted(n for n, _ in decl) == NAMES
    assert exports(hip_optim.LIB_PATH) == NAMES
    assert sorted(hip_optim.SIGNATURES) == NAMES
    for n, params in decl:
        assert [p for p, _ in hip_optim.SIGNATURES[n][1]] == params, n            # the header's names in the header's order
        assert len(getattr(L, n).argtypes) == len(params)
    assert L.dtc_optim_target_arch() == b"gfx950"
    with open(HEADER) as f:
        text = f.read()
    macro = lambda m: int(re.search(r"#define %s (\d+)" % m, text).group(1))
    assert (macro("DTC_SGD_MAX_TENSORS"), macro("DTC_SGD_MAX_ELEMENTS"), macro("DTC_SGD_MAX_TOTAL"), macro("DTC_SGD_MAX_GROUPS"),
            macro("DTC_SGD_CHUNK"), macro("DTC_SGD_BODY_CHUNKS"), macro("DTC_SGD_SKIP_NONFINITE")) == \
        (hip_optim.MAX_TENSORS, hip_optim.MAX_ELEMENTS, hip_optim.MAX_TOTAL, hip_optim.MAX_GROUPS, hip_optim.CHUNK,
         hip_optim.BODY_CHUNKS, hip_optim.SKIP_NONFINITE) == (16384, 1 << 30, 1 << 34, 64, 4096, 2048, 1)
    assert (orf.CHUNK, orf.BODY_CHUNKS) == (hip_optim.CHUNK, hip_optim.BODY_CHUNKS)
    fields = re.search(r"typedef struct dtc_sgd_tensor \{(.*?)\}", re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [n for n, _ in hip_optim.SgdTensor._fields_]
    assert C.sizeof(hip_optim.SgdTensor) == 40
    flags = open(os.path.join(ROOT, "detectorch_amd", "build.py")).read()
    assert "-ffp-contract=off" in flags and "build_optim" in flags


def test_other_libraries_exports_unchanged():
    from make_native_host_codes import exports
    from detectorch_amd import hip, hip_grad, hip_loss, hip_train
    with open(os.path.join(GOLDEN, "native_host_codes.json")) as f:
        want = json.load(f)["exports"]
    got = exports(hip.LIB_PATH)
    assert got == want and len(got) == 42 and not [n for n in got if "sgd" in n or "optim" in n]
    hip_train.lib()
    assert exports(hip_train.LIB_PATH) == ["dtc_fast_rcnn_targets", "dtc_train_target_arch"]
    hip_loss.lib()
    assert exports(hip_loss.LIB_PATH) == sorted(hip_loss.SIGNATURES) and len(hip_loss.SIGNATURES) == 5
    hip_grad.lib()
    assert exports(hip_grad.LIB_PATH) == ["dtc_grad_target_arch", "dtc_roi_align_backward", "dtc_roi_align_backward_workspace_bytes"]


# ---- the host functions, from a child process that sees no device -------------------------------------------------------------------
BASE = 1 << 20                                                        # a bogus, non-NULL, 16-byte aligned device address
BIG = 1 << 30

# label -> (overrides of _plan_call, expected code).  -1 DTC_EINVAL, -3 DTC_EWORKSPACE, -4 DTC_EUNSUPPORTED
PLAN_CODES = {
    "ok": (dict(), 0), "ok one element": (dict(counts=[1]), 0), "ok 64 groups": (dict(n_groups=64), 0),
    "ok p, g, buf back to back": (dict(counts=[5], p=[BASE], g=[BASE + 20], buf=[BASE + 40]), 0),
    "ok 2^30 elements": (dict(counts=[BIG], stride=1 << 34), 0), "ok 2^34 in all": (dict(counts=[BIG] * 16, stride=1 << 34), 0),
    "records NULL": (dict(records=None), -1), "n_chunks NULL": (dict(n_chunks=None), -1), "n_tensors 0": (dict(n_tensors=0), -1),
    "n_groups 0": (dict(n_groups=0), -1), "n 0": (dict(counts=[5, 0, 7]), -1), "n -3": (dict(counts=[-3]), -1),
    "group -1": (dict(groups=[0, -1, 0]), -1), "group == n_groups": (dict(groups=[0, 2, 0]), -1),
    # shapes before limits, limits before pointers, pointers before the size of plan_out
    "n_tensors 16385": (dict(counts=[1] * 16385), -4), "n 2^30 + 1": (dict(counts=[BIG + 1], stride=1 << 34), -4),
    "total 2^34 + 1": (dict(counts=[BIG] * 16 + [1], stride=1 << 34), -4), "n_groups 65": (dict(n_groups=65), -4),
    "n_groups 65 + n 0": (dict(n_groups=65, counts=[0]), -1), "n 2^30 + 1 + p NULL": (dict(counts=[BIG + 1], p=[0]), -4),
    "n_groups 65 + plan_out NULL": (dict(n_groups=65, plan_out=None), -4),
    "p NULL": (dict(counts=[5], p=[0]), -1), "g NULL": (dict(counts=[5], g=[0]), -1), "buf NULL": (dict(counts=[5], buf=[0]), -1),
    "p misaligned": (dict(counts=[5], p=[BASE + 2]), -1), "g misaligned": (dict(counts=[5], g=[BASE + 4097]), -1),
    "buf misaligned": (dict(counts=[5], buf=[BASE + 8195]), -1), "g is p": (dict(counts=[5], g=[BASE]), -1),
    "buf overlaps the end of p": (dict(counts=[5], buf=[BASE + 16]), -1),
    "p of one tensor inside g of another": (dict(counts=[100, 5], p=[BASE, BASE + (1 << 24) + 40]), -1),
    "plan_out NULL": (dict(plan_out=None), -1), "p NULL + plan short": (dict(counts=[5], p=[0], short=1), -1),
    "plan short": (dict(short=1), -3), "plan empty": (dict(short=10 ** 9), -3),
}

# label -> (overrides of _step_call, expected code)
STEP_CODES = {
    "n_tensors 0": (dict(n_tensors=0), -1), "n_chunks < n_tensors": (dict(n_chunks=2), -1), "n_groups 0": (dict(n_groups=0), -1),
    "plan_bytes one short": (dict(plan_bytes=3 * 32 + 5 * 16 - 1), -1), "plan_bytes one long": (dict(plan_bytes=3 * 32 + 5 * 16 + 1), -1),
    "max_norm 0": (dict(max_norm=0.0), -1), "max_norm -1": (dict(max_norm=-1.0), -1), "max_norm nan": (dict(max_norm=float("nan")), -1),
    "momentum 1": (dict(momentum=1.0), -1), "momentum -0.1": (dict(momentum=-0.1), -1), "momentum nan": (dict(momentum=float("nan")), -1),
    "flags 2": (dict(flags=2), -1),
    "n_tensors 16385": (dict(n_tensors=16385, n_chunks=16385, plan_bytes=16385 * 48), -4),
    "n_chunks > n_tensors + 2048": (dict(n_chunks=3 + 2049, plan_bytes=3 * 32 + 2052 * 16), -4), "n_groups 65": (dict(n_groups=65), -4),
    "n_groups 65 + max_norm 0": (dict(n_groups=65, max_norm=0.0), -1), "n_groups 65 + stats NULL": (dict(n_groups=65, stats=None), -4),
    "plan NULL": (dict(plan_dev=None), -1), "hyper NULL": (dict(group_hyper_dev=None), -1), "stats NULL": (dict(stats=None), -1),
    "plan misaligned": (dict(plan_dev=BASE + 8), -1), "hyper misaligned": (dict(group_hyper_dev=BASE + 2), -1),
    "stats misaligned": (dict(stats=BASE + 1), -1), "workspace misaligned": (dict(workspace=BASE + 8), -1),
    "stats NULL + workspace NULL": (dict(stats=None, workspace=None), -1),
    "workspace NULL": (dict(workspace=None), -3), "workspace short": (dict(workspace_bytes=47), -3),
}

TABLES = {"one": [1], "edges": [3, orf.CHUNK - 1, orf.CHUNK, orf.CHUNK + 1, 2 * orf.CHUNK + 1],
          "grown": [orf.CHUNK * orf.BODY_CHUNKS, 1, 3 * orf.CHUNK + 7], "many": [1 + (7 * k) % 5000 for k in range(300)],
          "large": [BIG, 5, BIG - 1, 1 << 29]}


def _plan_call(ho, counts=(5, 5000, 100), groups=None, n_groups=2, n_tensors=None, stride=1 << 24, short=0, table=False, **kw):
    """dtc_sgd_plan on records at bogus addresses -> (code, plan_out and *n_chunks untouched on an error | the table)"""
    n = len(counts)
    recs = (ho.SgdTensor * max(n, 1))()
    for k in range(n):
        at = BASE + 3 * k * stride
        recs[k] = ho.SgdTensor(kw["p"][k] if k < len(kw.get("p", ())) else at, kw["g"][k] if k < len(kw.get("g", ())) else at + stride,
                               kw["buf"][k] if k < len(kw.get("buf", ())) else at + 2 * stride, counts[k],
                               groups[k] if groups else k % min(max(n_groups, 1), 2), 0)
    L = ho.lib()
    need = L.dtc_sgd_plan_bytes(n, (C.c_int64 * max(n, 1))(*counts))
    size = max(need, 32 * n + 16 * n + 64)
    out = np.full(size, 0xFF, np.uint8)
    n_chunks = C.c_int(-77)
    rc = L.dtc_sgd_plan(None if "records" in kw else recs, n if n_tensors is None else n_tensors, n_groups,
                        None if "plan_out" in kw else out.ctypes.data, max(need - short, 0),
                        None if "n_chunks" in kw else C.byref(n_chunks))
    if rc != 0:
        return rc, bool(np.all(out == 0xFF)) and n_chunks.value == -77
    K = n_chunks.value
    need, bound = 32 * n + 16 * K, need
    assert need <= bound and np.all(out[need:] == 0xFF)
    t = out[:32 * n].view(np.dtype([("p", "<u8"), ("g", "<u8"), ("buf", "<u8"), ("n", "<u4"), ("group", "<i4")]))
    assert [(int(r["p"]), int(r["g"]), int(r["buf"]), int(r["n"]), int(r["group"])) for r in t] == \
        [(recs[k].p, recs[k].g, recs[k].buf, recs[k].n, recs[k].group) for k in range(n)]
    c = out[32 * n:need].view("<u4").reshape(K, 4)
    assert not c[:, 3].any()
    return rc, (c[:, :3].tolist() if table else True)


def _step_call(ho, n_tensors=3, n_chunks=5, n_groups=2, plan_bytes=3 * 32 + 5 * 16, momentum=0.9, max_norm=35.0, flags=0,
               workspace_bytes=48, **kw):
    v = lambda k: None if kw.get(k, BASE) is None else C.c_void_p(kw.get(k, BASE))
    return ho.lib().dtc_sgd_step(v("plan_dev"), plan_bytes, n_tensors, n_chunks, v("group_hyper_dev"), n_groups, momentum, max_norm,
                                 flags, v("workspace"), workspace_bytes, v("stats"), None)


def _child():
    from detectorch_amd import hip_optim as ho
    L = ho.lib()
    plan = {k: _plan_call(ho, **kw) for k, (kw, _) in PLAN_CODES.items()}
    counts = lambda c: (C.c_int64 * len(c))(*c)
    sizes = {"plan_bytes": {k: L.dtc_sgd_plan_bytes(len(c), counts(c)) for k, c in TABLES.items()},
             "plan_bytes_bad": [L.dtc_sgd_plan_bytes(0, counts([1])), L.dtc_sgd_plan_bytes(1, None), L.dtc_sgd_plan_bytes(1, counts([0])),
                                L.dtc_sgd_plan_bytes(1, counts([BIG + 1])), L.dtc_sgd_plan_bytes(17, counts([BIG] * 17)),
                                L.dtc_sgd_plan_bytes(16385, counts([1] * 16385))],
             "workspace": [L.dtc_sgd_workspace_bytes(k) for k in (-1, 0, 1, 2, 3, 2048, 16384 + 2048, 16384 + 2049)]}
    return dict(plan={k: [v[0], v[1]] for k, v in plan.items()}, step={k: _step_call(ho, **kw) for k, (kw, _) in STEP_CODES.items()},
                tables={k: _plan_call(ho, counts=c, stride=1 << 34, table=True)[1] for k, c in TABLES.items()}, sizes=sizes)


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return json.loads(out.stdout.decode())


def test_plan_return_codes_in_order(child):
    assert {k: v[0] for k, v in child["plan"].items()} == {k: v[1] for k, v in PLAN_CODES.items()}
    assert all(v[1] for v in child["plan"].values())                  # nothing written on an error; the records copied on success


def test_step_return_codes_in_order(child):
    assert child["step"] == {k: v[1] for k, v in STEP_CODES.items()}


def test_chunk_table_against_the_restatement(child):
    for name, counts in TABLES.items():
        got = [tuple(r) for r in child["tables"][name]]
        assert got == orf.chunk_table(counts), name
        # what the restatement itself must satisfy: every element exactly once, in order, no chunk across a tensor, K bounded
        at = {i: 0 for i in range(len(counts))}
        for i, off, cnt in got:
            assert off == at[i] and cnt >= 1
            at[i] += cnt
        assert [at[i] for i in range(len(counts))] == list(counts)
        assert len(counts) <= len(got) <= len(counts) + orf.BODY_CHUNKS
        bound = len(counts) + min(-(-sum(counts) // orf.CHUNK), orf.BODY_CHUNKS)
        assert child["sizes"]["plan_bytes"][name] == 32 * len(counts) + 16 * bound >= 32 * len(counts) + 16 * len(got)
    assert orf.chunk_elems(sum(TABLES["edges"])) == orf.CHUNK and orf.chunk_elems(sum(TABLES["grown"])) == 2 * orf.CHUNK
    assert max(c for _, _, c in orf.chunk_table(TABLES["large"])) == orf.chunk_elems(sum(TABLES["large"])) > BIG // 2048


def test_sizes_are_monotone(child):
    assert child["sizes"]["plan_bytes_bad"] == [0] * 6
    assert child["sizes"]["workspace"] == [0, 0, 16, 16, 32, 2048 * 8, (16384 + 2048) * 8, 0]
    from detectorch_amd import hip_optim as ho
    L = ho.lib()
    pb = lambda c: L.dtc_sgd_plan_bytes(len(c), (C.c_int64 * len(c))(*c))
    last = 0
    for n in (1, 2, orf.CHUNK, orf.CHUNK + 1, 10 * orf.CHUNK, orf.CHUNK * orf.BODY_CHUNKS, orf.CHUNK * orf.BODY_CHUNKS + 1, 1 << 30):
        now = pb([n, 7])                                              # growing one count never shrinks the buffer, although
        assert now >= last and now > 0                                # the chunk count itself drops where the chunk doubles
        last = now
        assert pb([n, 7, 1]) >= now
    ws = [L.dtc_sgd_workspace_bytes(k) for k in range(1, 200)]
    assert ws == sorted(ws) and all(w % 16 == 0 and w >= 8 * (k + 1) for k, w in enumerate(ws))


# ---- the restatement against torch itself -------------------------------------------------------------------------------------------
def test_restatement_equals_torch_in_float64():
    from detectorch_amd import synth
    rs = synth.rng(61, 0)
    shapes = [(7,), (64, 9), (1,), (33, 31), (512,), (40, 40), (275,)]
    assert len(shapes) == 7 and sum(int(np.prod(s)) for s in shapes) <= 4096
    groups = [0, 0, 1, 0, 1, 1, 0]
    hyper = [(0.05, 1e-4), (0.01, 0.0)]                               # the second group without weight decay
    momentum, max_norm = 0.9, 35.0
    p0 = [rs.standard_normal(s) for s in shapes]
    # norms on both sides of max_norm: the scale of the gradients alternates
    grads = [[rs.standard_normal(s) * (4.0 if step % 2 else 0.05) for s in shapes] for step in range(5)]
    tp = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p0]
    opt = torch.optim.SGD([dict(params=[t for t, k in zip(tp, groups) if k == g], lr=hyper[g][0], weight_decay=hyper[g][1])
                           for g in (0, 1)], lr=1.0, momentum=momentum)
    p = [a.copy() for a in p0]
    buf = [np.zeros_like(a) for a in p0]
    engaged = set()
    for step in range(5):
        for t, g in zip(tp, grads[step]):
            t.grad = torch.tensor(g, dtype=torch.float64)
        assert not any((g * 1.0 + 0.0 == 0).any() for g in grads[step])      # no zero update: the first-step -0.0 cannot occur
        torch.nn.utils.clip_grad_norm_(tp, max_norm)
        opt.step()
        total, coef = orf.step64(p, grads[step], buf, hyper, groups, momentum, max_norm)
        engaged.add(coef < 1.0)
        assert abs(total - orf.norm64(grads[step])) <= 1e-12 * total
        for a, t, b in zip(p, tp, buf):
            np.testing.assert_allclose(a, t.detach().numpy(), rtol=1e-11, atol=0)
            np.testing.assert_allclose(b, opt.state[t]['momentum_buffer'].numpy(), rtol=1e-11, atol=0)
    assert engaged == {True, False}
    # and the float32 restatement is the same step: within float32 rounding of the yardstick after one step
    q = [a.astype(np.float32) for a in p0]
    qb = [np.zeros_like(a) for a in q]
    g32 = [g.astype(np.float32) for g in grads[1]]
    orf.step32(q, g32, qb, orf.coef32(np.float32(orf.norm64(g32)), max_norm), hyper, groups, momentum)
    r = [a.astype(np.float32).astype(np.float64) for a in p0]
    rb = [np.zeros_like(a) for a in r]
    orf.step64(r, [g.astype(np.float64) for g in g32], rb, hyper, groups, momentum, max_norm)
    for a, b in zip(q, r):
        assert np.max(np.abs(a - b)) <= 8 * orf.EPS32 * max(1.0, np.max(np.abs(b)))
    assert orf.coef32(np.float32(35.0), 35.0) == np.float32(1) and np.isnan(orf.coef32(np.float32("nan"), 35.0))
    assert orf.coef32(np.float32("inf"), 35.0) == 0 and orf.coef32(np.float32(3.0), float("inf")) == 1


# ---- the Python surface on the CPU --------------------------------------------------------------------------------------------------
def _cpu_params(seed):
    torch.manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]


def test_state_dict_round_trips_with_torch_sgd():
    from detectorch_amd.optim import ClippedSGD
    a, b = _cpu_params(1), _cpu_params(1)
    ours = ClippedSGD([dict(params=a[:1]), dict(params=a[1:], lr=0.02, weight_decay=0.0)], lr=0.01)
    theirs = torch.optim.SGD([dict(params=b[:1]), dict(params=b[1:], lr=0.5, weight_decay=0.3)], lr=0.7, momentum=0.5, weight_decay=0.2)
    bufs = [torch.full_like(t, 1.5 + k) for k, t in enumerate(b)]
    theirs.state[b[0]]['momentum_buffer'] = bufs[0]                   # the reference's checkpoint: one buffer there, one missing
    theirs.state[b[1]]['momentum_buffer'] = None
    sd = theirs.state_dict()
    assert set(sd["param_groups"][0]) == set(ours.state_dict()["param_groups"][0])       # SGD's group keys, nothing else
    ours.load_state_dict(sd)
    assert [g['lr'] for g in ours.param_groups] == [0.7, 0.5] and [g['weight_decay'] for g in ours.param_groups] == [0.2, 0.3]
    assert ours.param_groups[0]['momentum'] == 0.5
    assert torch.equal(ours.state[a[0]]['momentum_buffer'], bufs[0]) and ours.state[a[1]].get('momentum_buffer') is None
    # ... and back: ours into a fresh torch SGD, which can then step
    ours.state[a[1]]['momentum_buffer'] = bufs[1].clone()
    back = torch.optim.SGD([dict(params=b[:1]), dict(params=b[1:])], lr=9.0)
    back.load_state_dict(ours.state_dict())
    assert [g['lr'] for g in back.param_groups] == [0.7, 0.5] and back.param_groups[1]['momentum'] == 0.5
    assert torch.equal(back.state[b[0]]['momentum_buffer'], bufs[0]) and torch.equal(back.state[b[1]]['momentum_buffer'], bufs[1])
    for t in b:
        t.grad = torch.ones_like(t)
    before = [t.detach().clone() for t in b]
    back.step()
    assert all(not torch.equal(x, t) for x, t in zip(before, b))
    assert ours.stats is None and ours.hyper is None                  # no step was taken, nothing touched a device


def test_constructor_checks():
    from detectorch_amd.optim import ClippedSGD
    for kw in (dict(lr=-1.0), dict(lr=0.1, momentum=1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, max_norm=0.0),
               dict(lr=0.1, max_norm=float("nan")), dict(lr=0.1, weight_decay=-1e-4)):
        with pytest.raises(ValueError):
            ClippedSGD(_cpu_params(2), **kw)
    assert ClippedSGD(_cpu_params(2), lr=0.1, max_norm=float("inf")).max_norm == float("inf")


def test_step_and_forward_train_raise_on_cpu_tensors():
    from detectorch_amd.model.detector import detector
    from detectorch_amd.optim import ClippedSGD
    params = _cpu_params(3)
    opt = ClippedSGD(params, lr=0.1)
    opt.step()                                                        # no gradient anywhere: nothing to do, nothing raised
    for t in params:
        t.grad = torch.ones_like(t)
    before = [t.detach().clone() for t in params]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert all(torch.equal(x, t) for x, t in zip(before, params))
    model = detector(N_classes=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.forward_train(torch.zeros(1, 3, 64, 96), torch.zeros(4, 5))
    with pytest.raises(NotImplementedError, match="inference-only"):
        detector(train=True)                                          # the constructor's refusal stays
    with pytest.raises(NotImplementedError, match="forward_train covers"):
        detector(N_classes=5, use_rpn_head=True).forward_train(torch.zeros(1, 3, 64, 96), torch.zeros(4, 5))


def test_freeze_stem_names_the_trainable_parameters():
    from detectorch_amd.model.detector import detector
    from detectorch_amd.train import freeze_stem
    model = detector(N_classes=5)
    trainable = freeze_stem(model)
    frozen = {n for n, p in model.named_parameters() if not p.requires_grad}
    assert frozen and all(n.startswith(("model.conv1.", "model.bn1.", "model.layer1.")) for n in frozen)
    assert all(not n.startswith(("model.conv1.", "model.bn1.", "model.layer1.")) for n, p in model.named_parameters() if p.requires_grad)
    assert len(trainable) == sum(p.requires_grad for p in model.parameters()) > 100
    assert model.model.layer2[0].conv1.weight.requires_grad and not model.model.layer1[0].conv1.weight.requires_grad


if __name__ == "__main__" and "--child" in sys.argv:
    print(json.dumps(_child()))
