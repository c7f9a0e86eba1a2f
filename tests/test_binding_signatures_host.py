"""The Python binding's signature tables against the C headers, without a GPU: every prototype of include/detectorch_hip.h and
include/detectorch_train_hip.h has one row in hip.SIGNATURES / hip_train.SIGNATURES with the same parameter names in the same order,
the matching kind per parameter and the matching return kind; lib() installs exactly those argtypes / restype; and the by-name call
helper orders, rejects and passes through as documented (against a stand-in library)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_INT = {"dtc_roi_align_get_exact", "launch_roi_align_forward_hip"}        # 0 = error (the reference's convention) / a value
SCALARS = {"int": "i", "float": "f", "size_t": "z", "long long": "q"}
RETURNS = {"const char*": "str", "size_t": "size", "void": "void"}
CTYPES = {"p": ctypes.c_void_p, "i": ctypes.c_int, "f": ctypes.c_float, "z": ctypes.c_size_t, "q": ctypes.c_longlong}
RESTYPES = {"status": ctypes.c_int, "int": ctypes.c_int, "size": ctypes.c_size_t, "str": ctypes.c_char_p, "void": None}


def prototypes(header):
    """{entry: (return kind, [(parameter, kind)])} of a header; kind: a letter of CTYPES, or the C name of a struct pointed to"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    src = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", src, flags=re.S)
    out = {}
    for ret, entry, params in re.findall(r"^([\w \*]+?)\b(dtc_\w+|launch_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        ret = ret.strip()
        kinds = []
        for p in [q.strip() for q in params.split(",") if q.strip() != "void"]:
            ctype, name = re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups()
            ctype = ctype.strip()
            if ctype.endswith("*"):
                pointee = ctype[:-1].replace("const", "").strip()
                kind = pointee if pointee.startswith("dtc_") else "p"
            else:
                kind = "p" if ctype == "dtc_stream_t" else SCALARS[ctype.replace("const", "").strip()]
            kinds.append((name, kind))
        out[entry] = (RETURNS.get(ret) or {"int": "int" if entry in PLAIN_INT else "status"}[ret], kinds)
    return out


def _struct_of(kind):
    """'dtc_feat_level' for the ctypes class whose docstring names that struct"""
    return re.match(r"struct (dtc_\w+)", kind.__doc__).group(1)


def _modules():
    from detectorch_amd import hip, hip_train
    return [(hip, "detectorch_hip.h", 42), (hip_train, "detectorch_train_hip.h", 2)]


def test_tables_equal_the_headers():
    for mod, header, count in _modules():
        protos = prototypes(header)
        assert sorted(mod.SIGNATURES) == sorted(protos) and len(protos) == count, header
        for entry, (ret, params) in protos.items():
            row = mod.SIGNATURES[entry]
            assert row[0] == ret, entry
            assert [n for n, _ in row[1]] == [n for n, _ in params], entry
            for (name, got), (_, want) in zip(row[1], params):
                assert (got if isinstance(got, str) else _struct_of(got)) == want, (entry, name)


def test_lib_installs_the_tables_types():
    for mod, _, _ in _modules():
        L = mod.lib()
        for entry, row in mod.SIGNATURES.items():
            fn = getattr(L, entry)
            want = [CTYPES[k] if isinstance(k, str) else ctypes.POINTER(k) for _, k in row[1]]
            assert list(fn.argtypes) == want and fn.restype == RESTYPES[row[0]], entry


class _StandIn:
    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.rc
        return fn


@pytest.fixture()
def stand_in(monkeypatch):
    from detectorch_amd import hip
    lib = _StandIn()
    monkeypatch.setattr(hip, "_lib", lib)
    monkeypatch.setattr(hip, "stream_ptr", lambda device=None: "current stream")
    return lib


def test_call_orders_keywords_converts_and_fills_the_stream(stand_in):
    import torch
    from detectorch_amd import hip
    dets, keep = torch.zeros(3, 5), torch.zeros(3, dtype=torch.int64)
    assert hip.call("dtc_nms", keep_count=None, workspace_bytes=True, n="3", keep_out=keep, thresh=1, dets=dets, workspace=None) == 0
    (name, args), = stand_in.calls
    assert name == "dtc_nms" and args == (dets.data_ptr(), 3, 1.0, None, 1, keep.data_ptr(), None, "current stream")
    assert [type(a) for a in args[1:5:3]] == [int, int] and type(args[2]) is float
    hip.call("dtc_nms", stream="mine", keep_count=None, workspace_bytes=0, n=3, keep_out=keep, thresh=0.5, dets=dets, workspace=None)
    assert stand_in.calls[1][1][-1] == "mine"
    stand_in.rc = 4096
    assert hip.call("dtc_nms_sorted_workspace_bytes", n_stride=7, n_seg=2) == 4096 and stand_in.calls[2] == ("dtc_nms_sorted_workspace_bytes", (2, 7))


def test_call_rejects_missing_and_unknown_names_before_the_library(stand_in):
    from detectorch_amd import hip
    with pytest.raises(TypeError, match="missing.*thresh"):
        hip.call("dtc_nms", dets=None, n=0, workspace=None, workspace_bytes=0, keep_out=None, keep_count=None)
    with pytest.raises(TypeError, match="unknown.*tresh"):
        hip.call("dtc_nms", dets=None, n=0, thresh=0.5, tresh=0.5, workspace=None, workspace_bytes=0, keep_out=None, keep_count=None)
    with pytest.raises(KeyError):
        hip.call("dtc_no_such_entry")
    assert stand_in.calls == []


def test_call_passes_structs_through_and_names_the_error(stand_in):
    from detectorch_amd import hip
    opt, scoring = hip.det_options(do_bbox_vote=True), hip.vote_scoring("AVG")
    levels = (hip.FeatLevel * 2)()
    hip.call("dtc_postprocess_detections_ex2_workspace_bytes", batch=1, max_rois=2, n_cls=3, opt=opt, scoring=scoring)
    hip.call("dtc_roi_align_forward_packed", levels=levels, n_levels=2, channels=4, in_dtype=0, roi_desc=None, n_rois=0, pooled_h=7,
             pooled_w=7, sampling_ratio=2, out=None, out_dtype=0)
    assert stand_in.calls[0][1][3] is opt and stand_in.calls[0][1][4] is scoring and stand_in.calls[1][1][0] is levels
    stand_in.rc = -4
    with pytest.raises(RuntimeError, match=r"roi_align\(box\) failed with DTC_EUNSUPPORTED"):
        hip.call("dtc_roi_align_forward_packed", "roi_align(box)", levels=levels, n_levels=2, channels=4, in_dtype=0, roi_desc=None,
                 n_rois=0, pooled_h=7, pooled_w=7, sampling_ratio=2, out=None, out_dtype=0)
    assert hip.call("dtc_roi_align_get_exact") == -4                           # a plain int is returned, not checked
