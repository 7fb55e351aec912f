"""Compare two bench.py --dump-outputs folders array by array, bit for bit.   usage: dump_outputs_cmp.py <dir a> <dir b> [label]"""
import glob
import os
import sys

import numpy as np

a_dir, b_dir = sys.argv[1], sys.argv[2]
label = sys.argv[3] if len(sys.argv) > 3 else ""
names = sorted({os.path.basename(p) for d in (a_dir, b_dir) for p in glob.glob(os.path.join(d, "*.npy"))})
bad = 0
for n in names:
    pa, pb = os.path.join(a_dir, n), os.path.join(b_dir, n)
    if not (os.path.exists(pa) and os.path.exists(pb)):
        print(f"{label} {n}: only in {'a' if os.path.exists(pa) else 'b'}"); bad += 1
        continue
    a, b = np.load(pa), np.load(pb)
    same = a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    print(f"{label} {n}: {a.dtype} {a.shape} {'bit-identical' if same else 'DIFFERENT'}")
    bad += not same
print(f"{label} {len(names)} arrays, {bad} different")
sys.exit(1 if bad or not names else 0)
