"""Builds the REFERENCE's own rasterizer kernels for gfx950 into oracle/_ref/libref_rasterizer.so -- test infrastructure, a recipe only.

The reference's three kernel sources (cuda_rasterizer/forward.cu, backward.cu, rasterizer_impl.cu) compile with hipcc once they see
  * oracle/ref_shim/: forwarding headers under the CUDA header names they include (cuda_runtime.h -> hip/hip_runtime.h,
    cooperative_groups.h -> hip/hip_cooperative_groups.h, cub/cub.cuh -> hipcub with `namespace cub = hipcub`) and the force-included
    ref_names.h, which maps the ten cuda* runtime names they use to their hip* twins;
  * the reference's vendored third_party/glm, which knows __HIP__;
  * one lexical rewrite on a build-time COPY: the sources spell their launches `<< <` ... `>> >`, which clang does not accept.
    `<< <` -> `<<<` and `>> >` -> `>>>` touch no arithmetic.
The kernels use no warp shuffles and no warp-size constant (16 x 16 blocks, __syncthreads_count, cub's scan and radix sort), so nothing in
them assumes 32-lane waves.  oracle/ref_capi.cpp (our own C ABI over CudaRasterizer::Rasterizer) is compiled with them.

-ffp-contract=off: the CPU oracle is built that way (oracle/Makefile) and the product's preprocess is bit-equal to the oracle, so whether
the reference binary and the oracle agree then rests on as few compiler choices as possible: the order of the operations as written, and
the device's sqrt / division / exp.  nvcc's own contraction choices could not be reproduced here in any case.

Nothing of the reference is kept: the copy lives in a temporary directory and is deleted; oracle/_ref/ (git-ignored) ends up holding the
library and manifest.json (compiler version, flags, SHA-256 of every reference source that went in).

    python oracle/ref_build.py [REFERENCE_ROOT]        # default: $GSRAST_REFERENCE_ROOT or /root/reference
"""
from __future__ import annotations

import concurrent.futures
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(_HERE, "_ref")
LIB_PATH = os.path.join(OUT_DIR, "libref_rasterizer.so")
MANIFEST_PATH = os.path.join(OUT_DIR, "manifest.json")
SHIM = os.path.join(_HERE, "ref_shim")
WRAPPER = os.path.join(_HERE, "ref_capi.cpp")
RAST = os.path.join("submodules", "gaussian_rasterization_ch3")
KERNEL_SOURCES = ("forward.cu", "backward.cu", "rasterizer_impl.cu")
FLAGS = ["--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off",
         "-Wno-unused-value"]      # (the reference ignores the hipError_t its cub / runtime calls return)
JOBS = 3


def reference_root(root: Optional[str] = None) -> Optional[str]:
    """The reference tree if it is on this machine, else None."""
    root = root or os.environ.get("GSRAST_REFERENCE_ROOT", "/root/reference")
    return root if os.path.isdir(os.path.join(root, RAST, "cuda_rasterizer")) else None


def _hipcc() -> str:
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _sha256(path: str) -> str:
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _recipe_files():
    return [os.path.abspath(__file__), WRAPPER] + sorted(glob.glob(os.path.join(SHIM, "**", "*.*"), recursive=True))


def _reference_files(root: str):
    d = os.path.join(root, RAST, "cuda_rasterizer")
    return sorted(glob.glob(os.path.join(d, "*.cu")) + glob.glob(os.path.join(d, "*.h")))


def up_to_date(root: str) -> bool:
    if not (os.path.exists(LIB_PATH) and os.path.exists(MANIFEST_PATH)):
        return False
    t = os.path.getmtime(LIB_PATH)
    return all(os.path.getmtime(p) <= t for p in _recipe_files() + _reference_files(root))


def build(root: Optional[str] = None, force: bool = False, verbose: bool = False) -> Optional[str]:
    """Library path, or None when there is no reference tree (then whatever oracle/_ref/ already holds is left alone)."""
    root = reference_root(root)
    if root is None:
        return None
    if not force and up_to_date(root):
        return LIB_PATH
    srcs = _reference_files(root)
    hipcc = _hipcc()
    tmp = tempfile.mkdtemp(prefix="ref_build_")
    try:
        for p in srcs:                              # the build-time copy, launch brackets rewritten
            with open(p, "r", encoding="utf-8", errors="surrogateescape") as f:
                text = f.read()
            with open(os.path.join(tmp, os.path.basename(p)), "w", encoding="utf-8", errors="surrogateescape") as f:
                f.write(text.replace("<< <", "<<<").replace(">> >", ">>>"))
        inc = ["-include", os.path.join(SHIM, "ref_names.h"), "-I", SHIM, "-I", tmp, "-I", os.path.join(root, RAST, "third_party", "glm")]
        units = [os.path.join(tmp, s) for s in KERNEL_SOURCES] + [WRAPPER]
        objs = [os.path.join(tmp, os.path.splitext(os.path.basename(u))[0] + ".o") for u in units]

        def compile_one(uo):
            cmd = [hipcc] + FLAGS + inc + ["-c", uo[0], "-o", uo[1]]
            if verbose:
                print("ref_build:", " ".join(cmd), flush=True)
            subprocess.check_call(cmd)

        with concurrent.futures.ThreadPoolExecutor(JOBS) as ex:
            list(ex.map(compile_one, zip(units, objs)))
        os.makedirs(OUT_DIR, exist_ok=True)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs)
        version = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.strip().splitlines()
        manifest = dict(compiler=version[:2], flags=FLAGS, rewrite=["<< < -> <<<", ">> > -> >>>"],
                        wrapper_sha256=_sha256(WRAPPER), sources={os.path.basename(p): _sha256(p) for p in srcs})
        with open(MANIFEST_PATH, "w") as f:
            json.dump(manifest, f, indent=1, sort_keys=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return LIB_PATH


def source_hashes() -> Optional[dict]:
    """The reference-source hashes of the library that is there (manifest.json), or None."""
    if not os.path.exists(MANIFEST_PATH):
        return None
    with open(MANIFEST_PATH) as f:
        return json.load(f)["sources"]


if __name__ == "__main__":
    _roots = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = build(_roots[0] if _roots else None, force="--force" in sys.argv, verbose=True)
    print("ref_build:", out if out else "no reference tree here, nothing built")
