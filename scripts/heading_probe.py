"""What does the device library's float64 atan2 return on lattice arguments?  torch.atan2 on the GPU against the exact model
(tests/atan2_exact.py): the 4225 half-integer pairs of tests/golden/atan2_lattice.npz, the 81 step vectors of the lattice walk
among them, and 20,000 random pairs of each kind of tests/test_atan2_exact.py (profiles/heading_device_atan2_probe.log).
usage: python scripts/heading_probe.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    from atan2_exact import atan2_cr
    from test_atan2_exact import random_pairs

    def report(name, y, x, want):
        got = torch.atan2(torch.from_numpy(np.ascontiguousarray(y)).cuda(), torch.from_numpy(np.ascontiguousarray(x)).cuda()).cpu().numpy()
        off = got.view(np.uint64) != want.view(np.uint64)
        ulps = np.abs(got.view(np.int64) - want.view(np.int64))[off]
        print(f"[probe] {name}: device differs from the model on {off.sum()} of {len(y)}; max {ulps.max() if off.any() else 0} ulp",
              flush=True)
        return off

    z = np.load(os.path.join(ROOT, "tests", "golden", "atan2_lattice.npz"))
    off = report("fixture (4225 half-integer pairs)", z["y"], z["x"], z["atan2"])
    for i in np.flatnonzero(off)[:12]:
        print("   ", z["y"][i], z["x"][i], repr(float(z["atan2"][i])))
    small = (np.abs(z["y"]) <= 2) & (np.abs(z["x"]) <= 2)
    print("[probe] of the 81 step vectors (|.|<=2):", int(off[small].sum()), "differ")
    for kind in ("f32", "f64"):
        y, x = random_pairs(kind, 20000)
        report("random " + kind, y, x, atan2_cr(y, x))


if __name__ == "__main__":
    main()
