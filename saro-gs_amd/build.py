"""Builds the gfx950 shared library (C ABI of include/gsrast.h) in-tree with hipcc.

The ROCm counterpart of the reference's setup.py (submodules/gaussian_rasterization_ch3/setup.py:17-33),
except that the product is a plain C-ABI .so loaded with ctypes, not a torch extension: no torch
headers are involved and the library has no Python dependency.

One object per translation unit of SOURCES, compiled side by side, linked into one library.  The tools that need another
build of the same sources take it from here, so the flags are written once:

    build.py [--force] [--out PATH] [-DNAME=VALUE ...]     # the library (PATH: a variant of it, tools/build_variant.sh)
    build.py --save-temps DIR [-DNAME=VALUE ...]           # objects + compiler temporaries into DIR; prints the gfx950 .s files
"""
from __future__ import annotations

import glob
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
SRC_DIR = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(HERE, "..", "include", "gsrast.h")
OUT = os.path.join(HERE, "diff_gaussian_rasterization_ch3", "libgsrast_hip.so")
OBJ_DIR = os.path.join(HERE, "build")      # (kept out of git: .gitignore)
SOURCES = ["gsrast_capi.hip", "gsrast_train.hip"]
MAX_JOBS = 16
FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    "-ffp-contract=off",                            # FMAs only where written: bit parity with the oracle
    "-fhip-fp32-correctly-rounded-divide-sqrt",     # IEEE divide / sqrt in the per-Gaussian kernels
    "-munsafe-fp-atomics",                          # hardware global_atomic_add_f32, no CAS loop
    "-fno-slp-vectorize",                           # packed fp32 VALU is half rate on gfx950 (tools/valu_calib.hip): SLP-formed v_pk_* plus the
                                                    # v_mov shuffles that feed them cost more than the scalar ops (blend_bwd -5 %)
    "-Wall", "-Wno-unused-function",
]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or put /opt/rocm/bin on PATH)")


def dependencies() -> list:
    """Every file the library is made from: all or nothing, any newer one rebuilds every unit."""
    return sorted(glob.glob(os.path.join(SRC_DIR, "*.h")) + glob.glob(os.path.join(SRC_DIR, "*.hip"))) + [INCLUDE, os.path.abspath(__file__)]


def needs_build(out: str = None) -> bool:
    out = out or OUT
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in dependencies())


def compile_units(obj_dir: str, extra_flags=(), verbose: bool = False) -> list:
    """Each unit of SOURCES -> obj_dir/<unit>.o, at most MAX_JOBS compilers at a time, run inside obj_dir (where -save-temps leaves its files)."""
    os.makedirs(obj_dir, exist_ok=True)
    jobs = []
    for f in SOURCES:
        obj = os.path.join(obj_dir, os.path.splitext(f)[0] + ".o")
        compile_flags = [x for x in FLAGS if x != "-shared"]      # (the one flag of FLAGS that only speaks to the link)
        jobs.append((obj, [hipcc()] + compile_flags + list(extra_flags) + ["-c", os.path.join(SRC_DIR, f), "-o", obj]))
    if verbose:
        for _, cmd in jobs:
            print(" ".join(cmd), file=sys.stderr)
    with ThreadPoolExecutor(max_workers=min(MAX_JOBS, len(jobs))) as pool:
        for r in [pool.submit(subprocess.check_call, cmd, cwd=obj_dir) for _, cmd in jobs]:
            r.result()
    return [obj for obj, _ in jobs]


def build(force: bool = False, verbose: bool = False, out: str = None, extra_flags=()) -> str:
    """out: another place for the library (a variant); extra_flags: appended to FLAGS for every unit and the link."""
    out = out or OUT
    if not force and not needs_build(out):
        return out
    objs = compile_units(os.path.join(OBJ_DIR, os.path.splitext(os.path.basename(out))[0]), extra_flags, verbose)
    cmd = [hipcc()] + FLAGS + list(extra_flags) + objs + ["-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def assembly(work_dir: str, extra_flags=()) -> list:
    """The gfx950 assembly of every unit (no GPU needed): compiled with -save-temps into work_dir; the .s files, one per unit."""
    compile_units(work_dir, list(extra_flags) + ["-save-temps"])
    return sorted(glob.glob(os.path.join(work_dir, "*gfx950*.s")))


if __name__ == "__main__":
    args = sys.argv[1:]
    paths = {k: os.path.abspath(args.pop(args.index(k) + 1)) for k in ("--out", "--save-temps") if k in args}
    extra = [a for a in args if a not in ("--force", "--out", "--save-temps")]      # (whatever else is given goes to the compiler)
    if "--save-temps" in paths:
        print("\n".join(assembly(paths["--save-temps"], extra)))
    else:
        print(build(force="--force" in args, verbose=True, out=paths.get("--out"), extra_flags=extra))
