"""Build libdetectorch_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m detectorch_amd.build [--force]

build_train() does the same for the training-side natives (csrc/train/*.hip -> libdetectorch_train_hip.so).

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


# ---- the training-side natives: a second library (include/detectorch_train_hip.h), so that the inference library's ABI stays as it is.
# sources() globs csrc/*.hip only; csrc/train/*.hip include the csrc/ headers by include path and are built with the same FLAGS.
TRAIN_CSRC = os.path.join(CSRC, "train")
TRAIN_LIB = os.path.join(LIBDIR, "libdetectorch_train_hip.so")


def train_sources():
    return sorted(glob.glob(os.path.join(TRAIN_CSRC, "*.hip")))


def needs_build_train():
    if not os.path.exists(TRAIN_LIB):
        return True
    t = os.path.getmtime(TRAIN_LIB)
    deps = (train_sources() + glob.glob(os.path.join(TRAIN_CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.h")) +
            glob.glob(os.path.join(HERE, "..", "include", "*.h")))
    return any(os.path.getmtime(d) > t for d in deps)


def build_train(force=False, verbose=False):
    if not force and not needs_build_train():
        return TRAIN_LIB
    objdir = os.path.join(LIBDIR, "obj_train")
    os.makedirs(objdir, exist_ok=True)
    cc = hipcc()
    objs = []
    for src in train_sources():                  # a handful of files: one after the other
        objs.append(os.path.join(objdir, os.path.basename(src)[:-4] + ".o"))
        cmd = [cc] + FLAGS + ["-I" + CSRC, "-c", src, "-o", objs[-1]]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    subprocess.check_call([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", TRAIN_LIB + ".tmp"] + objs)
    os.replace(TRAIN_LIB + ".tmp", TRAIN_LIB)
    return TRAIN_LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print(build_train(force="--force" in sys.argv, verbose=True))
