"""Build libdetectorch_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m detectorch_amd.build [--force]

build_train() does the same for the training-side natives (csrc/train/*.hip -> libdetectorch_train_hip.so), build_loss() for
the head losses and their gradients (csrc/loss/*.hip -> libdetectorch_loss_hip.so), build_grad() for the gradients of the region
operators (csrc/grad/*.hip -> libdetectorch_grad_hip.so), build_optim() for the optimizer tail of the training step
(csrc/optim/*.hip -> libdetectorch_optim_hip.so), build_rpn() for RPN training: anchor targets and the fused RPN losses
(csrc/rpn_train/*.hip -> libdetectorch_rpn_hip.so), build_mask() for mask training: mask targets and the fused mask loss
(csrc/mask_train/*.hip -> libdetectorch_mask_hip.so), build_eval() for scoring: COCO box AP and proposal recall
(csrc/eval/*.hip -> libdetectorch_eval_hip.so), build_segm() for scoring masks: RLE mask IoU and the match on it
(csrc/segm_eval/*.hip -> libdetectorch_segm_hip.so), build_poly() for ground-truth polygons at image size to run lists
(csrc/poly_rle/*.hip -> libdetectorch_poly_hip.so), build_flip() for the horizontal-flip augmentation: mirrored network input, boxes,
polygons and run lists (csrc/flip/*.hip -> libdetectorch_flip_hip.so), build_mpost() for mask post-processing on run lists: mask
boxes, mask overlaps, mask NMS and mask voting (csrc/mask_post/*.hip -> libdetectorch_mpost_hip.so), build_aug() for test-time
augmentation: the merge of the views' box-head outputs and the combination of their mask probabilities (csrc/aug/*.hip ->
libdetectorch_aug_hip.so), build_kps() for keypoint inference: heatmaps to keypoints (csrc/kps/*.hip -> libdetectorch_kps_hip.so).

No torch headers, no hipify, no multi-arch: one code object for gfx950.  -ffp-contract=off is part of the numerics
contract (see csrc/dtc_common.h).
"""
import glob
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libdetectorch_hip.so")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden",
         "-Wall", "-Wno-unused-function"]


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (need ROCm)")


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = sources() + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(HERE, "..", "include", "*.h"))
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    if not force and not needs_build():
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    cc = hipcc()
    procs = []
    objs = []
    for src in sources():
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        cmd = [cc] + FLAGS + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    failed = False
    for src, pr in procs:
        out, _ = pr.communicate()
        if pr.returncode != 0 or (verbose and out):
            sys.stderr.write(out.decode())
        failed |= pr.returncode != 0
    if failed:
        raise RuntimeError("hipcc failed")
    cmd = [cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB + ".tmp"] + objs
    subprocess.check_call(cmd)
    os.replace(LIB + ".tmp", LIB)
    return LIB


# ---- the side libraries, so that the inference library's ABI stays as it is: the training-side natives (include/detectorch_train_hip.h),
# the head losses with their gradients (include/detectorch_loss_hip.h), the gradients of the region operators
# (include/detectorch_grad_hip.h), the clipped SGD step (include/detectorch_optim_hip.h), RPN training
# (include/detectorch_rpn_hip.h), mask training (include/detectorch_mask_hip.h), scoring (include/detectorch_eval_hip.h), scoring
# masks (include/detectorch_segm_hip.h), polygons to run lists (include/detectorch_poly_hip.h), the horizontal flip
# (include/detectorch_flip_hip.h), mask post-processing (include/detectorch_mpost_hip.h) and test-time augmentation
# (include/detectorch_aug_hip.h), keypoint inference (include/detectorch_kps_hip.h; csrc/kps/*.hip).  sources()
# globs csrc/*.hip only; csrc/train/*.hip, csrc/loss/*.hip, csrc/grad/*.hip, csrc/optim/*.hip, csrc/rpn_train/*.hip, csrc/mask_train/*.hip,
# csrc/eval/*.hip, csrc/segm_eval/*.hip, csrc/poly_rle/*.hip, csrc/flip/*.hip, csrc/mask_post/*.hip and csrc/aug/*.hip include the csrc/ headers by include path and are built with the same
# FLAGS, one library per directory.
TRAIN_CSRC = os.path.join(CSRC, "train")
TRAIN_LIB = os.path.join(LIBDIR, "libdetectorch_train_hip.so")
LOSS_CSRC = os.path.join(CSRC, "loss")
LOSS_LIB = os.path.join(LIBDIR, "libdetectorch_loss_hip.so")
GRAD_CSRC = os.path.join(CSRC, "grad")
GRAD_LIB = os.path.join(LIBDIR, "libdetectorch_grad_hip.so")
OPTIM_CSRC = os.path.join(CSRC, "optim")
OPTIM_LIB = os.path.join(LIBDIR, "libdetectorch_optim_hip.so")
RPN_CSRC = os.path.join(CSRC, "rpn_train")
RPN_LIB = os.path.join(LIBDIR, "libdetectorch_rpn_hip.so")
MASK_CSRC = os.path.join(CSRC, "mask_train")
MASK_LIB = os.path.join(LIBDIR, "libdetectorch_mask_hip.so")
EVAL_CSRC = os.path.join(CSRC, "eval")                       # scoring (include/detectorch_eval_hip.h): COCO box AP, proposal recall
EVAL_LIB = os.path.join(LIBDIR, "libdetectorch_eval_hip.so")
SEGM_CSRC = os.path.join(CSRC, "segm_eval")                  # scoring masks (include/detectorch_segm_hip.h): RLE mask IoU, segm matching
SEGM_LIB = os.path.join(LIBDIR, "libdetectorch_segm_hip.so")
POLY_CSRC = os.path.join(CSRC, "poly_rle")                   # gt polygons at image size to run lists (include/detectorch_poly_hip.h): annToRLE
POLY_LIB = os.path.join(LIBDIR, "libdetectorch_poly_hip.so")
FLIP_CSRC = os.path.join(CSRC, "flip")                       # horizontal-flip augmentation (include/detectorch_flip_hip.h): input blob, boxes, polygons, RLE
FLIP_LIB = os.path.join(LIBDIR, "libdetectorch_flip_hip.so")
MPOST_CSRC = os.path.join(CSRC, "mask_post")                 # mask post-processing on run lists (include/detectorch_mpost_hip.h): boxes, overlaps, NMS, voting
MPOST_LIB = os.path.join(LIBDIR, "libdetectorch_mpost_hip.so")
AUG_CSRC = os.path.join(CSRC, "aug")                         # test-time augmentation (include/detectorch_aug_hip.h): merge of the views' boxes, combination of their masks
AUG_LIB = os.path.join(LIBDIR, "libdetectorch_aug_hip.so")
KPS_CSRC = os.path.join(CSRC, "kps")                         # keypoint inference (include/detectorch_kps_hip.h): heatmaps to keypoints
KPS_LIB = os.path.join(LIBDIR, "libdetectorch_kps_hip.so")


def _side_sources(csrc):
    return sorted(glob.glob(os.path.join(csrc, "*.hip")))


def _needs_side_build(lib, csrc):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    deps = (_side_sources(csrc) + glob.glob(os.path.join(CSRC, "*", "*.h")) + glob.glob(os.path.join(CSRC, "*.h")) +
            glob.glob(os.path.join(HERE, "..", "include", "*.h")))
    return any(os.path.getmtime(d) > t for d in deps)


def _build_side(lib, csrc, force, verbose):
    if not force and not _needs_side_build(lib, csrc):
        return lib
    objdir = os.path.join(LIBDIR, "obj_" + os.path.basename(csrc))
    os.makedirs(objdir, exist_ok=True)
    cc = hipcc()
    objs = []
    for src in _side_sources(csrc):              # a handful of files: one after the other
        objs.append(os.path.join(objdir, os.path.basename(src)[:-4] + ".o"))
        cmd = [cc] + FLAGS + ["-I" + CSRC, "-c", src, "-o", objs[-1]]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    subprocess.check_call([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib + ".tmp"] + objs)
    os.replace(lib + ".tmp", lib)
    return lib


def train_sources():
    return _side_sources(TRAIN_CSRC)


def needs_build_train():
    return _needs_side_build(TRAIN_LIB, TRAIN_CSRC)


def build_train(force=False, verbose=False):
    return _build_side(TRAIN_LIB, TRAIN_CSRC, force, verbose)


def build_loss(force=False, verbose=False):
    return _build_side(LOSS_LIB, LOSS_CSRC, force, verbose)


def build_grad(force=False, verbose=False):
    return _build_side(GRAD_LIB, GRAD_CSRC, force, verbose)


def build_optim(force=False, verbose=False):
    return _build_side(OPTIM_LIB, OPTIM_CSRC, force, verbose)


def build_rpn(force=False, verbose=False):
    return _build_side(RPN_LIB, RPN_CSRC, force, verbose)


def build_mask(force=False, verbose=False):
    return _build_side(MASK_LIB, MASK_CSRC, force, verbose)


def build_eval(force=False, verbose=False):
    return _build_side(EVAL_LIB, EVAL_CSRC, force, verbose)


def build_segm(force=False, verbose=False):
    return _build_side(SEGM_LIB, SEGM_CSRC, force, verbose)


def build_poly(force=False, verbose=False):
    return _build_side(POLY_LIB, POLY_CSRC, force, verbose)


def build_flip(force=False, verbose=False):
    return _build_side(FLIP_LIB, FLIP_CSRC, force, verbose)


def build_mpost(force=False, verbose=False):
    return _build_side(MPOST_LIB, MPOST_CSRC, force, verbose)


def build_aug(force=False, verbose=False):
    return _build_side(AUG_LIB, AUG_CSRC, force, verbose)


def build_kps(force=False, verbose=False):
    return _build_side(KPS_LIB, KPS_CSRC, force, verbose)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print(build_train(force="--force" in sys.argv, verbose=True))
    print(build_loss(force="--force" in sys.argv, verbose=True))
    print(build_grad(force="--force" in sys.argv, verbose=True))
    print(build_optim(force="--force" in sys.argv, verbose=True))
    print(build_rpn(force="--force" in sys.argv, verbose=True))
    print(build_mask(force="--force" in sys.argv, verbose=True))
    print(build_eval(force="--force" in sys.argv, verbose=True))
    print(build_segm(force="--force" in sys.argv, verbose=True))
    print(build_poly(force="--force" in sys.argv, verbose=True))
    print(build_flip(force="--force" in sys.argv, verbose=True))
    print(build_mpost(force="--force" in sys.argv, verbose=True))
    print(build_aug(force="--force" in sys.argv, verbose=True))
    print(build_kps(force="--force" in sys.argv, verbose=True))
