"""Generate tests/golden/roi_align_backward.npz from the REFERENCE ITSELF (build container only; needs the reference tree and g++).

    python tests/golden/make_roi_align_backward_golden.py [reference root, default /root/reference]

The reference's lib/cppcuda/roi_align_backward_cpu.cpp is compiled UNMODIFIED, where it lies, into a temporary directory
(g++ -O2 -ffp-contract=off -fno-fast-math -std=c++11) against a stand-in ATen/NativeFunctions.h written below -- AT_CHECK and an
at::Tensor with just the members that file uses -- and a short extern "C" driver that calls at::contrib::roi_align_backward_cpu.
Its results on the seeded cases of tests/roi_align_backward_ref.py are recorded and the build is deleted; nothing of the
reference's text is kept.

Per case <c> of roi_align_backward_ref.GOLDEN_CASES: <c>_digest (sha1 of the inputs), <c>_L<l> the float32 gradient of level l
[B, C', H, W] -- every channel, or for the cases of SAMPLED_CASES the channels sample_channels() names -- and <c>_e_ref, the
reference's own distance from the float64 yardstick in units of eps * sum|terms| (the maximum over the elements).  A multi-level
case is run as the contract says: the reference once per level on the RoIs of that level; 4-column RoIs get the zero batch column
that the reference's preprocess_rois (lib/model/roi_align.py:172-187) gives them.  e_ref: the maximum over the cases, without
"fsmall", whose terms are denormal (there the rounding quantum is the absolute 2^-149, not eps times the term).
The file is written with fixed zip timestamps: a second run gives the same bytes.
"""
import ctypes as C
import io
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import roi_align_backward_ref as rb  # noqa: E402

STAND_IN = r"""
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <vector>
#define AT_CHECK(cond, ...) do { if (!(cond)) std::abort(); } while (0)
namespace at {
struct Tensor;
struct Type { Tensor tensor(std::initializer_list<int64_t> sizes) const; };
struct Tensor {
  std::shared_ptr<std::vector<float> > store;
  std::vector<int64_t> sizes;
  Tensor() {}
  Tensor(const float* p, std::initializer_list<int64_t> s) : sizes(s) {
    int64_t n = 1;
    for (int64_t v : sizes) n *= v;
    store = std::make_shared<std::vector<float> >(p, p + n);
  }
  int64_t ndimension() const { return (int64_t)sizes.size(); }
  int64_t size(int64_t d) const { return sizes[d]; }
  int64_t numel() const { return (int64_t)store->size(); }
  bool is_contiguous() const { return true; }
  Type type() const { return Type(); }
  Tensor& zero_() { std::fill(store->begin(), store->end(), 0.f); return *this; }
  template <typename T> T* data() const { return store->data(); }
};
inline Tensor Type::tensor(std::initializer_list<int64_t> sizes) const {
  Tensor t;
  t.sizes = sizes;
  int64_t n = 1;
  for (int64_t v : sizes) n *= v;
  t.store = std::make_shared<std::vector<float> >(n);
  return t;
}
}  // namespace at
"""

DRIVER = r"""
#include "ATen/NativeFunctions.h"
namespace at { namespace contrib {
Tensor roi_align_backward_cpu(const Tensor&, const Tensor&, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, double, int64_t);
} }
extern "C" void run(const float* rois, long n_rois, const float* top, long batch, long channels, long height, long width, long ph,
                    long pw, double scale, long ratio, float* out) {
  at::Tensor r(rois, {n_rois, 5}), g(top, {n_rois, channels, ph, pw});
  at::Tensor o = at::contrib::roi_align_backward_cpu(r, g, batch, channels, height, width, ph, pw, scale, ratio);
  std::memcpy(out, o.data<float>(), sizeof(float) * (size_t)o.numel());
}
"""


def build_reference(ref_root, tmp):
    os.makedirs(os.path.join(tmp, "ATen"))
    with open(os.path.join(tmp, "ATen", "NativeFunctions.h"), "w") as f:
        f.write(STAND_IN)
    with open(os.path.join(tmp, "driver.cpp"), "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "libref_backward.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++11", "-shared", "-fPIC", "-I" + tmp,
                           os.path.join(ref_root, "lib", "cppcuda", "roi_align_backward_cpu.cpp"), os.path.join(tmp, "driver.cpp"),
                           "-o", so])
    L = C.CDLL(so)
    L.run.restype = None
    L.run.argtypes = [C.c_void_p, C.c_long, C.c_void_p] + [C.c_long] * 6 + [C.c_double, C.c_long, C.c_void_p]
    return L


def run_reference(L, top, rois5, batch, height, width, scale, ratio):
    top, rois5 = np.ascontiguousarray(top, np.float32), np.ascontiguousarray(rois5, np.float32)
    n, ch, ph, pw = top.shape
    out = np.full((batch, ch, height, width), np.nan, np.float32)
    L.run(rois5.ctypes.data, n, top.ctypes.data, batch, ch, height, width, ph, pw, float(scale), ratio, out.ctypes.data)
    return out


def write_npz(path, arrs):
    """np.load-compatible, with fixed timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrs[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    tmp = tempfile.mkdtemp(prefix="roi_align_backward_ref_")
    arrs, worst = {}, 0.0
    try:
        L = build_reference(ref_root, tmp)
        for name in rb.GOLDEN_CASES:
            c = rb.make_case(name)
            ch = rb.sample_channels(name, c["top"].shape[1])
            top = np.ascontiguousarray(c["top"][:, ch])
            rois = c["rois"] if c["rois"].shape[1] == 5 else np.hstack([np.zeros((len(c["rois"]), 1), np.float32), c["rois"]])
            levels = np.zeros(len(rois), np.int64) if c["levels"] is None else c["levels"]
            yard = rb.reference(c, ch)
            e_case, same = 0.0, True
            for l, ((h, w), s) in enumerate(zip(c["shapes"], c["scales"])):
                rows = np.where(levels == l)[0]
                got = run_reference(L, top[rows], rois[rows], c["batch"], h, w, s, c["ratio"])
                arrs["%s_L%d" % (name, l)] = got
                r32, y64, mag = yard[l]
                same &= np.array_equal(got.view(np.uint32), r32.view(np.uint32))
                with np.errstate(invalid="ignore", divide="ignore"):
                    e = np.abs(got.astype(np.float64) - y64) / (rb.EPS * mag)
                e_case = max(e_case, float(np.nanmax(np.where(mag > 0, e, 0.0))))
            arrs[name + "_digest"] = rb.digest(c)
            arrs[name + "_e_ref"] = np.float64(e_case)
            if name != "fsmall":
                worst = max(worst, e_case)
            print("%-7s top %-18s levels %d  e_ref %.3f eps*sum|terms|  restatement == reference: %s"
                  % (name, top.shape, len(c["shapes"]), e_case, same))
        arrs["e_ref"] = np.float64(worst)
        print("e_ref (maximum over the cases with normal terms): %.3f" % worst)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(HERE, "roi_align_backward.npz")
    write_npz(path, arrs)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(arrs)))


if __name__ == "__main__":
    main()
