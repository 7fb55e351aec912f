#!/usr/bin/env python3
"""Generate tests/golden/atan2_lattice.npz: every pair (y, x) of half-integers with |y|, |x| <= 16 (65 x 65 = 4225
pairs, the axes and (0, 0) included) and atan2(y, x) from mpmath at 200 bits, rounded once to double.

What is pinned, and by what: tests/atan2_exact.py (the correctly rounded heading, in Python integers) against an
independent multi-precision library.  mpmath is needed only here; the tests read the .npz file.  Its version goes into
the file.  Run in the BUILD container only:  python tests/golden/gen_atan2_lattice.py
"""
import os

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    mpmath.mp.prec = 200
    g = np.arange(-32, 33) * 0.5
    y, x = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    value = np.array([float(mpmath.atan2(mpmath.mpf(float(b)), mpmath.mpf(float(a)))) for b, a in zip(y, x)])
    out = os.path.join(HERE, "atan2_lattice.npz")
    np.savez_compressed(out, y=y, x=x, atan2=value, mpmath_version=np.array(mpmath.__version__), prec=np.array(200))
    print(f"{out}: {len(y)} pairs, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
