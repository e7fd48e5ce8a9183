"""The fp32 floor of the forward bars of tests/test_gpu_independent.py (no GPU needed): max |oracle32 - fp64 math| of the colour,
1 - final_T and the median depth over the unambiguous pixels of each case -- the HIP forward is bit-equal to the fp32 oracle in exp
mode 0.  The test's COLOUR_FLOOR / ALPHA_FLOOR are the largest values this prints; its docstring holds the table."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "saro-gs_amd"), os.path.join(ROOT, "tests")]
import scenes                                  # noqa: E402
import test_gpu_independent as T               # noqa: E402
from oracle import oracle as orc               # noqa: E402

orc.build()
orc.set_exp_mode(0)
print("case                       colour (max|ref|)     1 - final_T   depth abs (max|ref|)  rel")
for c in T.CASES:
    r = T._reference(scenes, c)
    o, _ = T._oracle32(orc, r)
    keep, out = r["keep"], r["out"]
    col, ref = o["out_color"].astype(np.float64), out["color"].detach().numpy()
    a, aref = (np.float32(1) - o["final_T"]).astype(np.float64), 1.0 - out["final_T"].detach().numpy()
    d, dref = o["out_depth"][0].astype(np.float64), out["depth"].numpy()
    print(f"{c['name']:26s} {np.abs(col - ref)[:, keep].max():.3g} ({np.abs(ref).max():.2g})   {np.abs(a - aref)[keep].max():.3g}   "
          f"{np.abs(d - dref)[keep].max():.3g} ({np.abs(dref).max():.2g})  {(np.abs(d - dref) / np.abs(dref))[keep].max():.2g}")
