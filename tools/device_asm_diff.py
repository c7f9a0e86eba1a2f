"""Device assembly of the working tree against a revision, function by function (CPU only: hipcc cross-compiles; about two minutes).

    python tools/device_asm_diff.py <rev> [file.hip ...]

For a change that is meant to leave every kernel as it is (a helper moved into a shared header, a host-side refactor).  Every
csrc/*.hip and csrc/train/*.hip of both trees -- or only the named ones -- is compiled with build.FLAGS + --cuda-device-only -S; one row
per file says whether the two assemblies are byte-identical, or hold the same functions with identical bodies (the compiler emits template
instantiations in the order they are first named, so moving a helper between headers can move them), or names the functions that
differ with their instruction counts.  Exit status 1 when a body or a function set differs.  It compares two trees; it does not
look at which instructions a kernel holds.
"""
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("detectorch_amd", "csrc")
MAX_COMPILES = 16


def load_build():      # build.py by path: its FLAGS and its hipcc(), without importing the package
    spec = importlib.util.spec_from_file_location("dtc_build", os.path.join(ROOT, "detectorch_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hip_files(tree):   # {"nms.hip": path, "train/fast_rcnn_targets.hip": path}
    out = {}
    for sub in ("", "train"):
        d = os.path.join(tree, CSRC, sub)
        for f in sorted(os.listdir(d)) if os.path.isdir(d) else []:
            if f.endswith(".hip"):
                out[os.path.join(sub, f)] = os.path.join(d, f)
    return out


def compile_asm(build, tree, src, dst):
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    cmd = [build.hipcc()] + build.FLAGS + ["-I" + os.path.join(tree, CSRC), "--cuda-device-only", "-S", src, "-o", dst]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s\n%s" % (src, r.stdout))
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", open(dst).read())


def functions(asm):
    """{symbol: [lines]}: from a function's .type directive to its .Lfunc_end label (the kernel descriptor lies in between) plus its
    `.set <symbol>.<resource>` lines; comments, blank space and the function index of local labels removed."""
    fns, cur = {}, None
    for line in asm.splitlines():
        line = line.split(";", 1)[0].strip()
        if not line:
            continue
        m = re.match(r"\.type\s+(\S+),@function$", line)
        if m:
            cur = fns.setdefault(m.group(1), [])
            continue
        m = re.match(r"\.set\s+(\S+)\.\w+,", line)
        if m and m.group(1) in fns:
            fns[m.group(1)].append(line)
            continue
        if cur is None:
            continue
        if re.match(r"\.Lfunc_end\d+:$", line):
            cur = None
            continue
        cur.append(re.sub(r"\.L([A-Za-z_]+?)\d+_(\d+)", r".L\1_\2", line))
    return fns


def n_instr(body):
    return sum(1 for l in body if not l.startswith(".") and not l.endswith(":"))


def demangle(names):
    if not names or not shutil.which("c++filt"):
        return list(names)
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(.*", "", n) for n in out]


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    rev, only = argv[1], set(argv[2:])
    build = load_build()
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "rev")
        os.makedirs(old)
        ar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", old], stdin=ar.stdout)
        if ar.wait() != 0:
            sys.exit("git archive %s failed" % rev)
        trees = {"rev": hip_files(old), "tree": hip_files(ROOT)}
        names = sorted(n for n in set(trees["rev"]) | set(trees["tree"]) if not only or os.path.basename(n) in only or n in only)
        jobs = {}
        with ThreadPoolExecutor(max_workers=min(MAX_COMPILES, os.cpu_count() or 1)) as pool:
            for side, root in (("rev", old), ("tree", ROOT)):
                for n in names:
                    if n in trees[side]:
                        jobs[side, n] = pool.submit(compile_asm, build, root, trees[side][n], os.path.join(tmp, "asm", side, n[:-4] + ".s"))
        bad = False
        for n in names:
            if (("rev", n) in jobs) != (("tree", n) in jobs):
                print("%-32s only in %s" % (n, rev if ("rev", n) in jobs else "the working tree"))
                bad = True
                continue
            a, b = jobs["rev", n].result(), jobs["tree", n].result()
            if a == b:
                print("%-32s byte-identical (%d lines)" % (n, a.count("\n")))
                continue
            fa, fb = functions(a), functions(b)
            gone, new = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
            diff = sorted(f for f in set(fa) & set(fb) if fa[f] != fb[f])
            if not (gone or new or diff):
                where = "emitted in another order" if list(fa) != list(fb) else "the file differs outside the bodies"
                print("%-32s the same %d functions, every body identical (%s)" % (n, len(fa), where))
                continue
            bad = True
            print("%-32s DIFFERS: %d of %d functions" % (n, len(diff), len(set(fa) & set(fb))))
            for f, d in zip(diff, demangle(diff)):
                print("    %s: %d -> %d instructions" % (d, n_instr(fa[f]), n_instr(fb[f])))
            for label, fs in (("only in " + rev, gone), ("only in the working tree", new)):
                for d in demangle(fs):
                    print("    %s: %s" % (label, d))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
