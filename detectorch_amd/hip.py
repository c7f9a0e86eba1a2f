"""ctypes binding of libdetectorch_hip.so (C ABI: include/detectorch_hip.h) + the torch plumbing around it.

PyTorch is used for device memory and the current HIP stream only; every computation below happens in the hand-written
HIP kernels of detectorch_amd/csrc.  There is NO fallback: if the library is missing this module raises on first use.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DETECTORCH_HIP_LIB") or os.path.join(_HERE, "lib", "libdetectorch_hip.so")

DTC_OK = 0
DTC_F32, DTC_F16, DTC_U8, DTC_BF16 = 0, 1, 2, 3
DTC_MAX_LEVELS = 8
_ERR = {-1: "DTC_EINVAL", -2: "DTC_ELAUNCH", -3: "DTC_EWORKSPACE", -4: "DTC_EUNSUPPORTED"}


class Image(C.Structure):
    """struct dtc_image (include/detectorch_hip.h)"""
    _fields_ = [("data", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("dtype", C.c_int32),
                ("row_stride", C.c_int32)]


class RpnLevel(C.Structure):
    """struct dtc_rpn_level (include/detectorch_hip.h)"""
    _fields_ = [("cls_prob", C.c_void_p), ("bbox_pred", C.c_void_p), ("num_anchors", C.c_int32), ("height", C.c_int32),
                ("width", C.c_int32), ("pre_nms_top_n", C.c_int32), ("feat_stride", C.c_float), ("score_is_logit", C.c_int32),
                ("anchors", C.c_float * 64)]


class FeatLevel(C.Structure):
    """struct dtc_feat_level (include/detectorch_hip.h)"""
    _fields_ = [("data", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("spatial_scale", C.c_float),
                ("_pad", C.c_int32), ("stride_n", C.c_int64), ("stride_c", C.c_int64), ("stride_h", C.c_int64),
                ("stride_w", C.c_int64)]


class FpnMapOut(C.Structure):
    """struct dtc_fpn_map_out (include/detectorch_hip.h)"""
    _fields_ = [("rois5", C.c_void_p), ("roi_levels", C.c_void_p), ("n_out", C.c_void_p), ("rois_by_level", C.c_void_p),
                ("level_counts", C.c_void_p), ("idx_restore", C.c_void_p), ("roi_order", C.c_void_p), ("roi_desc", C.c_void_p),
                ("k_min", C.c_int32), ("k_max", C.c_int32)]


class DetOptions(C.Structure):
    """struct dtc_det_options (include/detectorch_hip.h)"""
    _fields_ = [("nms_method", C.c_int32), ("soft_sigma", C.c_float), ("soft_score_thresh", C.c_float),
                ("bbox_vote", C.c_int32), ("bbox_vote_thresh", C.c_float)]


SOFT_NMS_METHODS = {"linear": 1, "gaussian": 2, "hard": 3}


def det_options(do_soft_nms=False, soft_nms_sigma=0.5, soft_nms_method='linear', do_bbox_vote=False, bbox_vote_thresh=0.8):
    """The reference's test-time options of box_results_with_nms_and_limit (lib/utils/result_utils.py:96-168) as a
    dtc_det_options, or None for the default (hard NMS, no voting).  The Soft-NMS score floor is the reference's 0.0001 (:138);
    voting is 'ID' scoring."""
    if not do_soft_nms and not do_bbox_vote:
        return None
    if do_soft_nms and soft_nms_method not in SOFT_NMS_METHODS:
        raise ValueError("Unknown soft_nms method: %s" % (soft_nms_method,))
    return DetOptions(SOFT_NMS_METHODS[soft_nms_method] if do_soft_nms else 0, float(soft_nms_sigma), 0.0001,
                      1 if do_bbox_vote else 0, float(bbox_vote_thresh))


class VoteScoring(C.Structure):
    """struct dtc_vote_scoring (include/detectorch_hip.h)"""
    _fields_ = [("method", C.c_int32), ("beta", C.c_float)]


# box_voting's scoring_method (lib/utils/boxes.py:280-329) -> DTC_VOTE_*
VOTE_METHODS = {"ID": 0, "TEMP_AVG": 1, "AVG": 2, "IOU_AVG": 3, "GENERALIZED_AVG": 4, "QUASI_SUM": 5}


def vote_scoring(method='ID', beta=1.0):
    """box_voting's scoring_method / beta as a dtc_vote_scoring, or None for 'ID' (the score is left as it is)."""
    if method not in VOTE_METHODS:
        raise NotImplementedError('Unknown scoring method {}'.format(method))               # boxes.py:324-327
    if method == 'ID':
        return None
    return VoteScoring(VOTE_METHODS[method], float(beta))


def det_options_scoring(options=None):
    """A region path's det_options dict (det_options' keywords + bbox_vote_method) -> (DetOptions or None, VoteScoring or
    None).  bbox_vote_method counts only with do_bbox_vote, as in box_results_with_nms_and_limit; an unknown one raises."""
    d = dict(options or {})
    scoring = vote_scoring(d.pop('bbox_vote_method', 'ID'))
    return det_options(**d), (scoring if d.get('do_bbox_vote') else None)


# One row per exported function of include/detectorch_hip.h: return kind, entry(parameter[:kind] ...), with the header's names in
# the header's order.  Return kinds: status (int DTC_* code, checked), int (plain: 0 can mean an error, the reference's convention),
# size (size_t), str (const char*), void.  Parameter kinds: a pointer (any T*, dtc_stream_t) unless marked i int, f float, z size_t,
# q long long, or with the ctypes class of a "const dtc_x*" struct pointer.  tests/test_binding_signatures_host.py holds the rows
# to the header.
_SIGNATURES = """
str dtc_version()
str dtc_target_arch()
int launch_roi_align_forward_hip(outputElements:i bottom_data bottom_rois spatial_scale:f channels:i height:i width:i
    pooled_height:i pooled_width:i sampling_ratio:i top_data stream)
status dtc_roi_align_forward(levels:FeatLevel n_levels:i channels:i in_dtype:i rois roi_cols:i roi_levels n_rois:i pooled_h:i
    pooled_w:i sampling_ratio:i out out_dtype:i stream)
status dtc_roi_align_forward_ordered(levels:FeatLevel n_levels:i channels:i in_dtype:i rois roi_cols:i roi_levels roi_order n_rois:i
    pooled_h:i pooled_w:i sampling_ratio:i out out_dtype:i stream)
status dtc_roi_align_forward_packed(levels:FeatLevel n_levels:i channels:i in_dtype:i roi_desc n_rois:i pooled_h:i pooled_w:i
    sampling_ratio:i out out_dtype:i stream)
size dtc_roi_align_workspace_bytes(n_rois:i)
void dtc_roi_align_set_exact(exact:i)
int dtc_roi_align_get_exact()
status dtc_roi_align_forward_packed_ws(levels:FeatLevel n_levels:i channels:i in_dtype:i roi_desc n_rois:i pooled_h:i pooled_w:i
    sampling_ratio:i out out_dtype:i workspace workspace_bytes:z stream)
size dtc_nms_workspace_bytes(n:i)
status dtc_nms(dets n:i thresh:f workspace workspace_bytes:z keep_out keep_count stream)
size dtc_nms_sorted_workspace_bytes(n_seg:i n_stride:i)
status dtc_nms_sorted(boxes counts n_seg:i n_stride:i thresh:f max_keep:i workspace workspace_bytes:z keep keep_stride:i keep_count
    stream)
status dtc_segment_sort_desc(scores score_stride_elems:i boxes box_stride_elems:i counts n_seg:i n_stride:i order sorted_boxes
    sorted_scores stream)
size dtc_rpn_topk_decode_workspace_bytes(levels:RpnLevel n_levels:i batch:i k_stride:i)
status dtc_rpn_topk_decode(levels:RpnLevel n_levels:i batch:i im_h:f im_w:f min_size_scaled:f workspace workspace_bytes:z out_boxes
    out_scores out_counts k_stride:i stream)
status dtc_rpn_topk_decode_sized(levels:RpnLevel n_levels:i batch:i im_h:f im_w:f im_hw min_size_scaled:f workspace
    workspace_bytes:z out_boxes out_scores out_counts k_stride:i stream)
status dtc_gather_kept(sorted_boxes sorted_scores n_seg:i k_stride:i keep keep_count keep_stride:i out_boxes out_scores stream)
status dtc_fpn_collect_distribute(in_boxes in_scores in_counts batch:i n_in_levels:i in_stride:i post_nms_top_n:i k_min:i k_max:i
    rois5 roi_scores roi_levels n_out rois_by_level level_counts idx_restore roi_order roi_desc inputs_sorted:i stream)
status dtc_fpn_collect_distribute_kept(sorted_boxes sorted_scores k_stride:i keep keep_count keep_stride:i batch:i n_in_levels:i
    post_nms_top_n:i k_min:i k_max:i rois5 roi_scores roi_levels n_out rois_by_level level_counts idx_restore roi_order roi_desc
    stream)
size dtc_prepare_proposals_workspace_bytes(batch:i max_out:i)
status dtc_prepare_proposals(boxes counts im_scale batch:i in_stride:i dedup_scale:f k_min:i k_max:i max_out:i workspace
    workspace_bytes:z rois5 roi_levels n_out rois_by_level level_counts idx_restore roi_order roi_desc src_index stream)
size dtc_postprocess_detections_workspace_bytes(batch:i max_rois:i n_cls:i)
status dtc_postprocess_detections(rois5 n_rois cls_score bbox_pred scaling_factor im_size batch:i max_rois:i n_cls:i wx:f wy:f ww:f
    wh:f score_thresh:f nms_thresh:f max_det:i workspace workspace_bytes:z dets det_roi det_rois_scaled det_count max_out:i stream)
status dtc_postprocess_detections_logits(rois5 n_rois cls_logits bbox_pred scaling_factor im_size batch:i max_rois:i n_cls:i wx:f
    wy:f ww:f wh:f score_thresh:f nms_thresh:f max_det:i workspace workspace_bytes:z dets det_roi det_rois_scaled det_count
    max_out:i stream)
status dtc_postprocess_detections_fpn(rois5 n_rois cls_score scores_are_logits:i bbox_pred scaling_factor im_size batch:i max_rois:i
    n_cls:i wx:f wy:f ww:f wh:f score_thresh:f nms_thresh:f max_det:i workspace workspace_bytes:z dets det_roi det_rois_scaled
    det_count max_out:i fpn:FpnMapOut stream)
status dtc_box_results_nms_limit(scores boxes n_rois batch:i max_rois:i n_cls:i score_thresh:f nms_thresh:f max_det:i workspace
    workspace_bytes:z dets det_roi det_count max_out:i stream)
size dtc_postprocess_detections_ex_workspace_bytes(batch:i max_rois:i n_cls:i opt:DetOptions)
status dtc_postprocess_detections_ex(rois5 n_rois cls_score scores_are_logits:i bbox_pred decoded_boxes scaling_factor im_size
    batch:i max_rois:i n_cls:i wx:f wy:f ww:f wh:f score_thresh:f nms_thresh:f max_det:i opt:DetOptions workspace workspace_bytes:z
    dets det_roi det_rois_scaled det_count max_out:i fpn:FpnMapOut stream)
size dtc_postprocess_detections_ex2_workspace_bytes(batch:i max_rois:i n_cls:i opt:DetOptions scoring:VoteScoring)
status dtc_postprocess_detections_ex2(rois5 n_rois cls_score scores_are_logits:i bbox_pred decoded_boxes scaling_factor im_size
    batch:i max_rois:i n_cls:i wx:f wy:f ww:f wh:f score_thresh:f nms_thresh:f max_det:i opt:DetOptions scoring:VoteScoring
    workspace workspace_bytes:z dets det_roi det_rois_scaled det_count max_out:i fpn:FpnMapOut stream)
status dtc_mask_paste(masks mask_index n_cls:i M:i dets det_count im_size batch:i max_out:i thresh_binarize:f cls_specific_mask:i
    crops per_image_capacity:q mask_boxes mask_rects mask_offsets mask_bytes stream)
status dtc_mask_rle(crops per_image_capacity:q mask_rects mask_offsets det_count im_size batch:i max_out:i rle_counts runs_stride:i
    rle_n_runs rle_str str_stride:i rle_str_len stream)
status dtc_bbox_overlaps(boxes n:i box_cols:i query_boxes k:i query_cols:i overlaps stream)
status dtc_box_voting(top_dets n_top:i all_dets n_all:i thresh:f top_dets_out n_voters stream)
status dtc_box_voting_scored(top_dets n_top:i all_dets n_all:i thresh:f scoring:VoteScoring top_dets_out n_voters stream)
status dtc_bias_act(x bias residual n:i c:i h:i w:i dtype:i channels_last:i relu:i residual_up2:i stream)
status dtc_prep_plan(heights widths batch:i target_size:i max_size:i pad_stride:i im_scales out_hw blob_hw)
status dtc_prep_images(images:Image batch:i pixel_means im_scales out_hw blob blob_h:i blob_w:i stream)
status dtc_soft_nms(dets n:i sigma:f overlap_thresh:f score_thresh:f method:i dets_out inds_out n_out stream)
status dtc_bbox_transform(boxes deltas n:i n_cls:i wx:f wy:f ww:f wh:f do_clip:i im_h:f im_w:f out stream)
"""

_KINDS = {"p": C.c_void_p, "i": C.c_int, "f": C.c_float, "z": C.c_size_t, "q": C.c_longlong, "d": C.c_double}
_RETURNS = {"status": C.c_int, "int": C.c_int, "size": C.c_size_t, "str": C.c_char_p, "void": None}


def _pointer(v):
    if type(v) is torch.Tensor:
        return v.data_ptr()
    data_ptr = getattr(v, "data_ptr", None)       # (a Parameter); None (NULL), a stream handle or a host ctypes array: itself
    return v if data_ptr is None else data_ptr()


def _as_is(v):
    return v


_CONVERT = {"p": _pointer, "i": int, "f": float, "z": int, "q": int, "d": float}


def signatures(rows, structs):
    """The rows of a signature table -> {entry: (return kind, ((parameter, kind), ...), ((parameter, invoke's converter), ...))}; a
    struct kind is its class in `structs`."""
    table = {}
    for row in rows.replace("\n    ", " ").strip().split("\n"):
        ret, entry, params = row.replace("(", " ").rstrip(")").split(" ", 2)
        params = tuple((n, k if k in _KINDS else structs[k]) for n, k in ((p + ":p").split(":")[:2] for p in params.split()))
        table[entry] = (ret, params, tuple((n, _CONVERT.get(k, _as_is)) for n, k in params))
    return table


SIGNATURES = signatures(_SIGNATURES, {c.__name__: c for c in (FeatLevel, RpnLevel, FpnMapOut, DetOptions, VoteScoring, Image)})


def typed(L, table):
    """Install the argtypes / restype of every entry of `table` on the CDLL L."""
    for entry, (ret, params, _) in table.items():
        fn = getattr(L, entry)
        fn.argtypes = [_KINDS[k] if k in _KINDS else C.POINTER(k) for _, k in params]
        fn.restype = _RETURNS[ret]
    return L


_lib = None


def lib():
    """Load the native library or fail loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                "There is no CPU/PyTorch fallback for the region-proposal hot path." % LIB_PATH)
        _lib = typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def check(rc, what):
    if rc != DTC_OK:
        raise RuntimeError("detectorch_hip: %s failed with %s" % (what, _ERR.get(rc, rc)))


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def invoke(L, table, entry, args, what=None):
    """L.entry with the keyword arguments `args` placed in the table's order; returns what it returns, a status entry's DTC_E* code
    raises instead (check), naming `what` or the entry.  Pointers: a tensor gives its data_ptr(), None is NULL; int / float kinds go
    through int() / float(); a ctypes struct or array is passed as the object it is.  A `stream` that is not given is the current
    stream of the current device.  TypeError, before the library is touched, on a missing or unknown name."""
    ret, params, convert = table[entry]
    if "stream" not in args and params and params[-1][0] == "stream":
        args["stream"] = stream_ptr()
    try:
        if len(args) != len(params):
            raise KeyError
        values = [c(args[n]) for n, c in convert]                  # (as many names as parameters and none missing: none unknown)
    except KeyError:
        names = [n for n, _ in params]
        raise TypeError("%s: missing %s, unknown %s" % (entry, [n for n in names if n not in args],
                                                        [n for n in args if n not in names])) from None
    rc = getattr(L, entry)(*values)
    if ret == "status":
        check(rc, what or entry)
    return rc


def call(entry, what=None, /, **args):
    """An entry of libdetectorch_hip.so by parameter name (invoke)."""
    return invoke(lib(), SIGNATURES, entry, args, what)


def _dtype_code(t):
    if t == torch.float32:
        return DTC_F32
    if t == torch.float16:
        return DTC_F16
    if t == torch.bfloat16:
        return DTC_BF16
    raise TypeError("detectorch_hip supports float32 / float16 / bfloat16 features, got %s" % t)


def _require_cuda(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("detectorch_amd runs the region-proposal hot path on the GPU only (got a CPU tensor); "
                               "there is no CPU fallback")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise TypeError("all tensors must be on the same device")
    return dev


def make_levels(features, spatial_scales):
    """list of [B,C,H,W] tensors (any strides: NCHW-contiguous or channels_last) -> (FeatLevel array, C, dtype)."""
    if len(features) > DTC_MAX_LEVELS:
        raise ValueError("at most %d levels" % DTC_MAX_LEVELS)
    arr = (FeatLevel * len(features))()
    ch, dt = features[0].shape[1], features[0].dtype
    for k, (t, s) in enumerate(zip(features, spatial_scales)):
        if t.dim() != 4 or t.shape[1] != ch or t.dtype != dt:
            raise ValueError("feature levels must be [B,C,H,W] with equal C and dtype")
        sn, sc, sh, sw = t.stride()
        arr[k] = FeatLevel(t.data_ptr(), t.shape[2], t.shape[3], float(s), 0, sn, sc, sh, sw)
    return arr, ch, dt


def bias_act_(x, bias=None, residual=None, relu=True, residual_up2=False):
    """dtc_bias_act: in place  x = act(x + bias[c] + residual)  on a dense [N,C,H,W] tensor (NCHW-contiguous or channels_last;
    float32 / float16 / bfloat16).  bias float32 [C]; residual of x's dtype and layout, [N,C,H,W] or -- residual_up2 --
    [N,C,H/2,W/2] read with nearest x2 upsampling (the FPN top-down sum).  Returns x."""
    dev = _require_cuda(x, bias, residual)
    if x.dim() != 4:
        raise ValueError("x must be [N,C,H,W]")
    n, c, h, w = x.shape
    if x.is_contiguous():
        cl = 0
    elif x.is_contiguous(memory_format=torch.channels_last):
        cl = 1
    else:
        raise ValueError("x must be dense (NCHW-contiguous or channels_last)")
    if bias is not None:
        if bias.dtype != torch.float32 or bias.numel() != c or not bias.is_contiguous():
            raise ValueError("bias must be a contiguous float32 [C] tensor")
    if residual is not None:
        want = (n, c, h // 2, w // 2) if residual_up2 else (n, c, h, w)
        if tuple(residual.shape) != want or residual.dtype != x.dtype:
            raise ValueError("residual must be %s of dtype %s" % (want, x.dtype))
        ok = residual.is_contiguous(memory_format=torch.channels_last) if cl else residual.is_contiguous()
        if not ok:
            raise ValueError("residual must have x's memory layout")
    elif residual_up2:
        raise ValueError("residual_up2 needs a residual")
    with torch.cuda.device(dev):      # like every other launcher: the kernel goes to x's device whatever the current one is
        call("dtc_bias_act", x=x, bias=bias, residual=residual, n=n, c=c, h=h, w=w, dtype=_dtype_code(x.dtype), channels_last=cl,
             relu=bool(relu), residual_up2=bool(residual_up2))
    return x


def roi_align_set_exact(exact=True):
    """Process-wide switch (dtc_roi_align_set_exact): True (default) = bit-identical to the reference; False = the C4 (adaptive
    sampling, single level) kernel may merge taps -- the same sums in exact arithmetic, <= 1e-5 from the reference in float32.
    Read by the host at LAUNCH time: a hipGraph keeps the mode it was captured with; shared by all threads / streams of the process
    (include/detectorch_hip.h)."""
    call("dtc_roi_align_set_exact", exact=bool(exact))


def roi_align_forward(features, spatial_scales, rois, pooled_h, pooled_w, sampling_ratio, roi_levels=None,
                      out_dtype=None, out=None, roi_order=None):
    """Multi-level RoIAlign forward (dtc_roi_align_forward).

    features: tensor or list of tensors [B,C,H_l,W_l]; rois [R,4|5] float32; roi_levels int32 [R] or None.
    Returns [R,C,PH,PW] in roi order.
    """
    if torch.is_tensor(features):
        features, spatial_scales = [features], [spatial_scales]
    dev = _require_cuda(rois, roi_levels, *features)
    if rois.dtype != torch.float32:
        raise TypeError("rois must be float32")
    rois = rois.contiguous()
    if (len(features) == 1 and features[0].shape[0] == 1 and rois.dim() == 2 and rois.shape[1] == 5 and rois.shape[0] > 0
            and roi_levels is None):
        # one image: the batch column can only hold 0 (lib/cppcuda/roi_align_cpu.cpp:143-147 indexes the batch with it), so the
        # RoIs go down as 4 columns -- which tells the library that they all belong to one map (map-stationary kernel for C4)
        rois = rois[:, 1:].contiguous()
    R, cols = (rois.shape[0], rois.shape[1]) if rois.dim() == 2 else (0, 5)
    lv, ch, dt = make_levels(features, spatial_scales)
    odt = out_dtype or (out.dtype if out is not None else torch.float32)
    if out is not None and (out.dtype != odt or not out.is_contiguous()):
        raise TypeError("out must be contiguous and of dtype out_dtype")
    if out is None:
        out = torch.empty((R, ch, pooled_h, pooled_w), dtype=odt, device=dev)
    if roi_levels is not None:
        roi_levels = roi_levels.to(torch.int32).contiguous()
    if roi_order is not None:
        roi_order = roi_order.to(torch.int32).contiguous()
    with torch.cuda.device(dev):
        call("dtc_roi_align_forward_ordered", "dtc_roi_align_forward", levels=lv, n_levels=len(features), channels=ch,
             in_dtype=_dtype_code(dt), rois=rois, roi_cols=cols if R else 5, roi_levels=roi_levels, roi_order=roi_order, n_rois=R,
             pooled_h=pooled_h, pooled_w=pooled_w, sampling_ratio=sampling_ratio, out=out, out_dtype=_dtype_code(odt))
    return out


def roi_align_packed(levels, channels, in_dtype, roi_desc, n_rois, pooled_h, pooled_w, sampling_ratio, out, ws=None, stream=None,
                     what="roi_align(packed)"):
    """dtc_roi_align_forward_packed -- with a workspace `ws`, dtc_roi_align_forward_packed_ws -- over a FeatLevel array (make_levels)
    of in_dtype maps: the rows of roi_desc [n_rois,8] into out [n_rois,channels,pooled_h,pooled_w], on `stream` (None: the current
    one).  No allocation and no device guard: the caller's."""
    args = dict(levels=levels, n_levels=len(levels), channels=channels, in_dtype=_dtype_code(in_dtype), roi_desc=roi_desc,
                n_rois=n_rois, pooled_h=pooled_h, pooled_w=pooled_w, sampling_ratio=sampling_ratio, out=out,
                out_dtype=_dtype_code(out.dtype), stream=stream or stream_ptr(out.device))
    if ws is None:
        call("dtc_roi_align_forward_packed", what, **args)
    else:
        call("dtc_roi_align_forward_packed_ws", what, workspace=ws, workspace_bytes=ws.numel(), **args)


def _ptr(t):
    return None if t is None else t.data_ptr()


def workspace(nbytes, device):
    """uint8 scratch tensor (torch owns the memory; the kernels only see the pointer)."""
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)


def nms(dets, thresh):
    """dtc_nms: dets [N,5] float32 CUDA tensor -> int64 CUDA tensor of ascending original indices (one D2H for the count)."""
    dev = _require_cuda(dets)
    n = dets.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.int64, device=dev)
    dets = dets.contiguous()
    if dets.dtype != torch.float32 or dets.dim() != 2 or dets.shape[1] != 5:
        raise TypeError("dets must be float32 [N,5]")
    ws = workspace(call("dtc_nms_workspace_bytes", n=n), dev)
    keep = torch.empty((n,), dtype=torch.int64, device=dev)
    cnt = torch.empty((1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("dtc_nms", dets=dets, n=n, thresh=thresh, workspace=ws, workspace_bytes=ws.numel(), keep_out=keep, keep_count=cnt)
    return keep[:int(cnt.item())]


def nms_sorted(boxes, counts, thresh, max_keep=0, keep_stride=None):
    """dtc_nms_sorted: boxes [S,N,4] score-sorted, counts int32 [S] or None -> (keep int32 [S,keep_stride], keep_count [S])."""
    dev = _require_cuda(boxes, counts)
    boxes = boxes.contiguous()
    S, N = boxes.shape[0], boxes.shape[1]
    ks = int(keep_stride or (max_keep if max_keep > 0 else N))
    ws = workspace(call("dtc_nms_sorted_workspace_bytes", n_seg=S, n_stride=N), dev)
    keep = torch.empty((S, max(ks, 1)), dtype=torch.int32, device=dev)
    cnt = torch.empty((max(S, 1),), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("dtc_nms_sorted", boxes=boxes, counts=counts, n_seg=S, n_stride=N, thresh=thresh, max_keep=max_keep, workspace=ws,
             workspace_bytes=ws.numel(), keep=keep, keep_stride=ks, keep_count=cnt)
    return keep, cnt[:S]


def make_rpn_levels(cls_probs, bbox_preds, anchors, feat_strides, pre_nms_top_n, scores_are_logits=False):
    """lists (one entry per level) of [B,A,H,W] / [B,4A,H,W] float32 CUDA tensors + base anchors [A,4] -> RpnLevel array.
    scores_are_logits: cls_probs holds the pre-sigmoid RPN logits (dtc_rpn_level.score_is_logit)."""
    n = len(cls_probs)
    arr = (RpnLevel * n)()
    keep_alive = []
    for k in range(n):
        c, d = cls_probs[k].contiguous(), bbox_preds[k].contiguous()
        if c.dtype != torch.float32 or d.dtype != torch.float32:
            raise TypeError("RPN outputs must be float32")
        B, A, H, W = c.shape
        if d.shape != (B, 4 * A, H, W):
            raise ValueError("rpn_bbox_pred must be [B,4A,H,W]")
        a = [float(v) for v in anchors[k].reshape(-1)]
        if len(a) != 4 * A or A > 16:
            raise ValueError("need A<=16 base anchors of 4 coordinates")
        lv = RpnLevel(c.data_ptr(), d.data_ptr(), A, H, W, int(pre_nms_top_n[k]), float(feat_strides[k]),
                      1 if scores_are_logits else 0)
        for q, v in enumerate(a):
            lv.anchors[q] = v
        arr[k] = lv
        keep_alive += [c, d]
    return arr, keep_alive


def generate_proposals(cls_probs, bbox_preds, anchors, feat_strides, im_h, im_w, pre_nms_top_n, post_nms_top_n,
                       nms_thresh, min_size_scaled=0.0, scores_are_logits=False, im_hw=None):
    """Batched multi-level GenerateProposals (generate_proposals.py:31-122) with zero host round trips.
    scores_are_logits=True folds the RPN head's sigmoid (detector.py:125) into the top-k: pass the raw logits, get the
    proposals and PROBABILITY scores the reference would produce from sigmoid(logits), without materialising them.

    Returns (boxes [B,L,P,4], scores [B,L,P], counts int32 [B,L]) with P = post_nms_top_n (rows >= count undefined),
    plus the pre-NMS (sorted) boxes/scores/counts for callers that want them.
    im_hw [B,2] (h_b, w_b) per image (dtc_rpn_topk_decode_sized): image b of the padded batch gives what a batch-1 call on its
    own (h_b, w_b) blob gives; None: every image is (im_h, im_w).
    """
    dev = _require_cuda(*cls_probs, *bbox_preds)
    nl = len(cls_probs)
    B = cls_probs[0].shape[0]
    lv, alive = make_rpn_levels(cls_probs, bbox_preds, anchors, feat_strides, pre_nms_top_n, scores_are_logits)
    kmax = 0
    for k in range(nl):
        N = cls_probs[k].shape[1] * cls_probs[k].shape[2] * cls_probs[k].shape[3]
        K = N if (pre_nms_top_n[k] <= 0 or pre_nms_top_n[k] >= N) else int(pre_nms_top_n[k])
        kmax = max(kmax, K)
    S = B * nl
    ws = workspace(call("dtc_rpn_topk_decode_workspace_bytes", levels=lv, n_levels=nl, batch=B, k_stride=kmax), dev)
    pre_boxes = torch.empty((S, kmax, 4), dtype=torch.float32, device=dev)
    pre_scores = torch.empty((S, kmax), dtype=torch.float32, device=dev)
    pre_counts = torch.empty((S,), dtype=torch.int32, device=dev)
    if im_hw is not None:
        im_hw = torch.as_tensor(im_hw, dtype=torch.float32).to(dev).reshape(B, 2).contiguous()
    with torch.cuda.device(dev):
        call("dtc_rpn_topk_decode_sized", levels=lv, n_levels=nl, batch=B, im_h=im_h, im_w=im_w, im_hw=im_hw,
             min_size_scaled=min_size_scaled, workspace=ws, workspace_bytes=ws.numel(), out_boxes=pre_boxes, out_scores=pre_scores,
             out_counts=pre_counts, k_stride=kmax)
    if nms_thresh <= 0:                                   # generate_proposals.py:114
        return (pre_boxes.view(B, nl, kmax, 4), pre_scores.view(B, nl, kmax), pre_counts.view(B, nl),
                pre_boxes, pre_scores, pre_counts)
    P = int(post_nms_top_n) if post_nms_top_n > 0 else kmax
    P = min(P, kmax)
    keep, kcnt = nms_sorted(pre_boxes, pre_counts, nms_thresh, max_keep=P, keep_stride=P)
    out_boxes = torch.empty((S, P, 4), dtype=torch.float32, device=dev)
    out_scores = torch.empty((S, P), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call("dtc_gather_kept", sorted_boxes=pre_boxes, sorted_scores=pre_scores, n_seg=S, k_stride=kmax, keep=keep, keep_count=kcnt,
             keep_stride=P, out_boxes=out_boxes, out_scores=out_scores)
    del alive
    return (out_boxes.view(B, nl, P, 4), out_scores.view(B, nl, P), kcnt.view(B, nl), pre_boxes, pre_scores, pre_counts)


def collect_outputs(B, T, n_levels, dev, scores=True):
    """The output set of dtc_fpn_collect_distribute / _kept / dtc_prepare_proposals for B images x T roi rows, under the entry points'
    parameter names and in their order (call(entry, ..., **outputs)): rois5 [B,T,5], roi_scores [B,T] (None without scores),
    roi_levels [B,T], n_out [B], rois_by_level [B,T,4], level_counts [B,n_levels], idx_restore [B,T], roi_order [B,T], roi_desc [B,T,8]."""
    f32, i32 = torch.float32, torch.int32
    e = lambda *shape, dtype=f32: torch.empty(shape, dtype=dtype, device=dev)
    return dict(rois5=e(B, T, 5), roi_scores=e(B, T) if scores else None, roi_levels=e(B, T, dtype=i32), n_out=e(B, dtype=i32),
                rois_by_level=e(B, T, 4), level_counts=e(B, n_levels, dtype=i32), idx_restore=e(B, T, dtype=i32),
                roi_order=e(B, T, dtype=i32), roi_desc=e(B, T, 8))


def det_outputs(B, D, dev, scaled=True):
    """The output set of the detection entries for B images x D rows, under dtc_postprocess_detections_ex2's parameter names and in
    their order: dets [B,D,6], det_roi [B,D], det_rois_scaled [B,D,4] (None without `scaled`: decoded boxes), det_count [B]."""
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    return dict(dets=z(B, D, 6), det_roi=z(B, D, dtype=torch.int32), det_rois_scaled=z(B, D, 4) if scaled else None,
                det_count=torch.empty((B,), dtype=torch.int32, device=dev))


def paste_outputs(B, D, crop_cols, dev):
    """The output set of dtc_mask_paste under its parameter names and in their order: crops uint8 [B,crop_cols], mask_boxes /
    mask_rects int32 [B,D,4], mask_offsets int64 [B,D], mask_bytes int64 [B]."""
    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device=dev)
    return dict(crops=torch.empty((B, crop_cols), dtype=torch.uint8, device=dev), mask_boxes=z(B, D, 4), mask_rects=z(B, D, 4),
                mask_offsets=z(B, D, dtype=torch.int64), mask_bytes=z(B, dtype=torch.int64))


def rle_outputs(B, D, runs_stride, str_stride, dev, zero_str=False):
    """The output set of dtc_mask_rle under its parameter names and in their order: rle_counts [B,D,runs_stride], rle_n_runs [B,D],
    rle_str uint8 [B,D,str_stride] (zero_str: cleared, for a path that reads it between steps), rle_str_len [B,D]."""
    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device=dev)
    return dict(rle_counts=torch.empty((B, D, runs_stride), dtype=torch.int32, device=dev), rle_n_runs=z(B, D),
                rle_str=(torch.zeros if zero_str else torch.empty)((B, D, str_stride), dtype=torch.uint8, device=dev),
                rle_str_len=z(B, D))


def fpn_collect_distribute(boxes, scores, counts, post_nms_top_n, k_min=2, k_max=5, inputs_sorted=False):
    """dtc_fpn_collect_distribute.  boxes [B,L,P,4], scores [B,L,P] or None, counts int32 [B,L].
    -> dict(rois5 [B,T,5], roi_scores, roi_levels [B,T], n_out [B], rois_by_level [B,T,4], level_counts [B,nl],
            idx_restore [B,T])"""
    dev = _require_cuda(boxes, scores, counts)
    boxes = boxes.contiguous()
    B, Lin, P = boxes.shape[0], boxes.shape[1], boxes.shape[2]
    T = int(post_nms_top_n)
    out = collect_outputs(B, T, k_max - k_min + 1, dev, scores=scores is not None)
    if scores is not None:
        scores = scores.contiguous()
    counts = counts.to(torch.int32).contiguous()
    with torch.cuda.device(dev):
        call("dtc_fpn_collect_distribute", in_boxes=boxes, in_scores=scores, in_counts=counts, batch=B, n_in_levels=Lin, in_stride=P,
             post_nms_top_n=T, k_min=k_min, k_max=k_max, inputs_sorted=bool(inputs_sorted), **out)
    return out


def prepare_proposals(boxes, counts, im_scale, dedup_scale=0.0625, k_min=2, k_max=5, max_out=None, out=None, ws=None):
    """dtc_prepare_proposals: precomputed proposals -> the outputs of fpn_collect_distribute (in_scores = NULL), one call for a batch.
    boxes float32 [B,N,4] in original-image coordinates, counts int32 [B] (rows past them ignored), im_scale [B] (rounded to
    float32 like numpy's float32-array * Python-float product); dedup_scale 0.0625 (remove_dup_prop) or 0 (keep every row in input
    order); k_min == k_max: one level (C4).  -> dict(rois5 [B,T,5], roi_levels [B,T], n_out [B], rois_by_level [B,T,4],
    level_counts [B,nl], idx_restore [B,T], roi_order [B,T], roi_desc [B,T,8], src_index [B,T]) with T = max_out (default N).
    out / ws: preallocated dict / workspace to write into (graph capture)."""
    dev = _require_cuda(boxes, counts)
    boxes = boxes.contiguous()
    B, N = boxes.shape[0], boxes.shape[1]
    T = int(max_out or N)
    f32, i32 = torch.float32, torch.int32
    if out is None:
        out = collect_outputs(B, T, k_max - k_min + 1, dev, scores=False)
        del out["roi_scores"]
        out["src_index"] = torch.empty((B, T), dtype=i32, device=dev)
    counts = counts.to(i32).contiguous()
    im_scale = torch.as_tensor(im_scale, dtype=f32).to(dev).reshape(B).contiguous()
    if ws is None:
        ws = workspace(call("dtc_prepare_proposals_workspace_bytes", batch=B, max_out=T), dev)
    outputs = dict({"src_index": None}, **out)               # a given `out` may lack src_index and may carry collect's roi_scores
    outputs.pop("roi_scores", None)
    with torch.cuda.device(dev):
        call("dtc_prepare_proposals", boxes=boxes, counts=counts, im_scale=im_scale, batch=B, in_stride=N, dedup_scale=dedup_scale,
             k_min=k_min, k_max=k_max, max_out=T, workspace=ws, workspace_bytes=ws.numel(), **outputs)
    return out


def det_workspace_bytes(batch, max_rois, n_cls, opt=None, bbox_vote_method='ID', scoring=None):
    """dtc_postprocess_detections_ex2_workspace_bytes (opt: a DetOptions or None; the vote scoring as a method name or, when
    given, a VoteScoring)"""
    if scoring is None:
        scoring = vote_scoring(bbox_vote_method)
    need = call("dtc_postprocess_detections_ex2_workspace_bytes", batch=batch, max_rois=max_rois, n_cls=n_cls, opt=opt, scoring=scoring)
    if need == 0:
        raise ValueError("invalid detection post-processing shape or options")
    return need


def _postprocess(scores, n_rois, rois5, deltas, decoded, sf, im_size, logits, weights, score_thresh, nms_thresh, max_det, max_out,
                 ws, do_soft_nms, soft_nms_sigma, soft_nms_method, do_bbox_vote, bbox_vote_thresh, bbox_vote_method):
    """dtc_postprocess_detections_ex2 on contiguous device tensors: scores [B,R,C] with either rois5 + deltas + sf + im_size (class
    decode in the kernel; det_rois_scaled is written) or decoded boxes [B,R,4C].  -> (dets, det_roi, det_scaled or None, det_count)"""
    dev = scores.device
    B, R, ncls = scores.shape
    if max_out is None:
        max_out = 128 if max_det > 0 else R * (ncls - 1)
    opt = det_options(do_soft_nms, soft_nms_sigma, soft_nms_method, do_bbox_vote, bbox_vote_thresh)
    scoring = vote_scoring(bbox_vote_method)
    need = det_workspace_bytes(B, R, ncls, opt, scoring=scoring)
    if ws is None or ws.numel() < need:
        ws = workspace(need, dev)
    out = det_outputs(B, max_out, dev, scaled=decoded is None)
    wx, wy, ww, wh = weights
    with torch.cuda.device(dev):
        call("dtc_postprocess_detections_ex2", rois5=rois5, n_rois=n_rois, cls_score=scores, scores_are_logits=bool(logits),
             bbox_pred=deltas, decoded_boxes=decoded, scaling_factor=sf, im_size=im_size, batch=B, max_rois=R, n_cls=ncls, wx=wx, wy=wy,
             ww=ww, wh=wh, score_thresh=score_thresh, nms_thresh=nms_thresh, max_det=max_det, opt=opt, scoring=scoring, workspace=ws,
             workspace_bytes=ws.numel(), max_out=max_out, fpn=None, **out)
    return tuple(out.values())


def postprocess_detections(rois5, n_rois, cls_score, bbox_pred, scaling_factor, im_size, weights=(10., 10., 5., 5.),
                           score_thresh=0.05, nms_thresh=0.5, max_det=100, max_out=None, ws=None, scores_are_logits=False,
                           do_soft_nms=False, soft_nms_sigma=0.5, soft_nms_method='linear', do_bbox_vote=False,
                           bbox_vote_thresh=0.8, bbox_vote_method='ID'):
    """dtc_postprocess_detections_ex2.  rois5 [B,R,5], cls_score [B,R,C], bbox_pred [B,R,4C], scaling_factor [B], im_size [B,2].
    scores_are_logits=True: cls_score holds the raw cls_score-layer output and the softmax of detector.py:281 is folded into
    the kernel; the probability map is never materialised.  do_soft_nms / soft_nms_sigma / soft_nms_method / do_bbox_vote /
    bbox_vote_thresh / bbox_vote_method: the reference's options of box_results_with_nms_and_limit (result_utils.py:96-168;
    bbox_vote_method is box_voting's scoring_method, beta 1.0 as there).
    -> (dets [B,max_out,6], det_roi [B,max_out], det_rois_scaled [B,max_out,4], det_count [B])"""
    _require_cuda(rois5, n_rois, cls_score, bbox_pred, scaling_factor, im_size)
    f32 = torch.float32
    return _postprocess(cls_score.contiguous(), n_rois, rois5.contiguous(), bbox_pred.contiguous(), None,
                        scaling_factor.to(f32).contiguous(), im_size.to(f32).contiguous(), scores_are_logits, weights, score_thresh,
                        nms_thresh, max_det, max_out, ws, do_soft_nms, soft_nms_sigma, soft_nms_method, do_bbox_vote,
                        bbox_vote_thresh, bbox_vote_method)


def box_results_nms_limit(scores, boxes, n_rois=None, score_thresh=0.05, nms_thresh=0.5, max_det=100, max_out=None, ws=None,
                          do_soft_nms=False, soft_nms_sigma=0.5, soft_nms_method='linear', do_bbox_vote=False, bbox_vote_thresh=0.8,
                          bbox_vote_method='ID'):
    """box_results_with_nms_and_limit on decoded boxes (dtc_postprocess_detections_ex2 with decoded_boxes): scores [B,R,C],
    decoded boxes [B,R,4C] -> (dets [B,max_out,6], det_roi [B,max_out], det_count [B]).  Options as postprocess_detections."""
    _require_cuda(scores, boxes, n_rois)
    dets, det_roi, _, det_count = _postprocess(scores.contiguous(), n_rois, None, None, boxes.contiguous(), None, None, False,
                                               (1., 1., 1., 1.), score_thresh, nms_thresh, max_det, max_out, ws, do_soft_nms,
                                               soft_nms_sigma, soft_nms_method, do_bbox_vote, bbox_vote_thresh, bbox_vote_method)
    return dets, det_roi, det_count


def mask_paste(masks, dets, det_count, im_size, M, per_image_capacity, mask_index=None, thresh=0.5, cls_specific=True):
    """dtc_mask_paste -> dict(crops uint8 [B,cap], boxes int32 [B,D,4], rects int32 [B,D,4], offsets int64 [B,D], bytes int64 [B])"""
    dev = _require_cuda(masks, dets, det_count, im_size, mask_index)
    masks, dets = masks.contiguous(), dets.contiguous()
    B, D = dets.shape[0], dets.shape[1]
    cap = int(per_image_capacity)
    out = paste_outputs(B, D, max(cap, 1), dev)
    with torch.cuda.device(dev):
        call("dtc_mask_paste", masks=masks, mask_index=mask_index, n_cls=masks.shape[1], M=M, dets=dets, det_count=det_count,
             im_size=im_size.to(torch.float32).contiguous(), batch=B, max_out=D, thresh_binarize=thresh,
             cls_specific_mask=bool(cls_specific), per_image_capacity=cap, **out)
    return {k.replace("mask_", ""): v for k, v in out.items()}


def mask_rle(paste, det_count, im_size, runs_stride=4096, str_stride=8192):
    """dtc_mask_rle on the dict returned by mask_paste -> dict(counts uint32 [B,D,runs_stride], n_runs int32 [B,D],
    str uint8 [B,D,str_stride], str_len int32 [B,D]).  Negative n_runs / str_len: that detection did not fit."""
    crops, rects, offs = paste["crops"], paste["rects"], paste["offsets"]
    dev = _require_cuda(crops, rects, offs, det_count, im_size)
    B, D = rects.shape[0], rects.shape[1]
    out = rle_outputs(B, D, int(runs_stride), int(str_stride), dev)
    with torch.cuda.device(dev):
        call("dtc_mask_rle", crops=crops, per_image_capacity=crops.shape[1], mask_rects=rects, mask_offsets=offs, det_count=det_count,
             im_size=im_size.to(torch.float32).contiguous(), batch=B, max_out=D, runs_stride=runs_stride, str_stride=str_stride, **out)
    return {k.replace("rle_", ""): v for k, v in out.items()}


def bbox_overlaps(boxes, query_boxes):
    """dtc_bbox_overlaps: [N,>=4], [K,>=4] float32 CUDA -> [N,K] float32 (cython_bbox.pyx:32-72)."""
    dev = _require_cuda(boxes, query_boxes)
    boxes, query_boxes = boxes.contiguous(), query_boxes.contiguous()
    n, k = boxes.shape[0], query_boxes.shape[0]
    out = torch.zeros((n, k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call("dtc_bbox_overlaps", boxes=boxes, n=n, box_cols=boxes.shape[1] if n else 4, query_boxes=query_boxes, k=k,
             query_cols=query_boxes.shape[1] if k else 4, overlaps=out)
    return out


def box_voting(top_dets, all_dets, thresh, scoring_method='ID', beta=1.0):
    """dtc_box_voting_scored: [T,5], [A,5] float32 CUDA -> ([T,5], n_voters int32 [T]); scoring_method / beta as box_voting's
    (lib/utils/boxes.py:280-329; 'ID' leaves column 4, the others write the voted score)."""
    scoring = vote_scoring(scoring_method, beta)
    dev = _require_cuda(top_dets, all_dets)
    top_dets, all_dets = top_dets.contiguous(), all_dets.contiguous()
    t, a = top_dets.shape[0], all_dets.shape[0]
    out = torch.empty((t, 5), dtype=torch.float32, device=dev)
    nv = torch.zeros((max(t, 1),), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("dtc_box_voting_scored", top_dets=top_dets, n_top=t, all_dets=all_dets, n_all=a, thresh=thresh, scoring=scoring,
             top_dets_out=out, n_voters=nv)
    return out, nv[:t]


def prep_images(images, pixel_means=(122.7717, 115.9465, 102.9801), target_size=800, max_size=1333, pad_stride=32):
    """dtc_prep_plan + dtc_prep_images: list of HWC BGR CUDA tensors (uint8 or float32, [h,w,3]) ->
    (blob float32 [B,3,Hb,Wb] on the device, im_scales list of float, resized sizes list of (h, w))."""
    dev = _require_cuda(*images)
    B = len(images)
    ims = [im if im.stride(2) == 1 and im.stride(1) == 3 else im.contiguous() for im in images]
    hs = (C.c_int32 * B)(*[int(im.shape[0]) for im in ims])
    ws_ = (C.c_int32 * B)(*[int(im.shape[1]) for im in ims])
    scales = (C.c_double * B)()
    out_hw = (C.c_int32 * (2 * B))()
    blob_hw = (C.c_int32 * 2)()
    call("dtc_prep_plan", heights=hs, widths=ws_, batch=B, target_size=target_size, max_size=max_size, pad_stride=pad_stride,
         im_scales=scales, out_hw=out_hw, blob_hw=blob_hw)
    arr = (Image * B)()
    for k, im in enumerate(ims):
        if im.dtype == torch.uint8:
            dt = 2
        elif im.dtype == torch.float32:
            dt = 0
        else:
            raise TypeError("images must be uint8 or float32")
        if im.dim() != 3 or im.shape[2] != 3:
            raise ValueError("images must be [h,w,3] (BGR)")
        arr[k] = Image(im.data_ptr(), int(im.shape[0]), int(im.shape[1]), dt, int(im.stride(0)))
    means = (C.c_double * 3)(*[float(m) for m in pixel_means])
    blob = torch.empty((B, 3, blob_hw[0], blob_hw[1]), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call("dtc_prep_images", images=arr, batch=B, pixel_means=means, im_scales=scales, out_hw=out_hw, blob=blob,
             blob_h=blob_hw[0], blob_w=blob_hw[1])
    del ims
    return blob, [float(s) for s in scales], [(out_hw[2 * k], out_hw[2 * k + 1]) for k in range(B)]


def soft_nms(dets, sigma, overlap_thresh, score_thresh, method):
    """dtc_soft_nms: dets [N,5] float32 CUDA -> (dets' [N',5], inds int64 [N'])."""
    dev = _require_cuda(dets)
    dets = dets.contiguous()
    n = dets.shape[0]
    out = torch.empty((max(n, 1), 5), dtype=torch.float32, device=dev)
    inds = torch.empty((max(n, 1),), dtype=torch.int64, device=dev)
    cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("dtc_soft_nms", dets=dets, n=n, sigma=sigma, overlap_thresh=overlap_thresh, score_thresh=score_thresh, method=method,
             dets_out=out, inds_out=inds, n_out=cnt)
    k = int(cnt.item())
    return out[:k], inds[:k]


def bbox_transform(boxes, deltas, weights, clip_to=None):
    """dtc_bbox_transform: boxes [N,4], deltas [N,4K] CUDA float32 -> [N,4K]; clip_to=(im_h, im_w) also clips."""
    dev = _require_cuda(boxes, deltas)
    boxes, deltas = boxes.contiguous(), deltas.contiguous()
    n, k = deltas.shape[0], deltas.shape[1] // 4
    out = torch.empty_like(deltas)
    (wx, wy, ww, wh), (im_h, im_w) = weights, clip_to if clip_to is not None else (0.0, 0.0)
    with torch.cuda.device(dev):
        call("dtc_bbox_transform", boxes=boxes, deltas=deltas, n=n, n_cls=k, wx=wx, wy=wy, ww=ww, wh=wh, do_clip=clip_to is not None,
             im_h=im_h, im_w=im_w, out=out)
    return out
