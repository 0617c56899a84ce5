#!/usr/bin/env python3
"""Golden paths for the MAS tie rule from the REAL reference function (jatts/modules/alignments.py: _monotonic_alignment_search):
    python tests/golden/make_golden_mas_ties.py <path of the reference checkout>  ->  tests/golden/mas_ties.npz
numba is absent: ``jit`` becomes the identity (exactly as make_golden_mas.py does it), so the reference's own statements run under numpy.

The inputs are the integer-coded kinds of tests/alignment_cases.py (q4, half, const) at its shapes up to (300, 257): every partial sum is exact in
f32 and f64 whatever its order, so the reference's float32 row-0 sums, the oracle's float64 ones and the kernel's agree to the last bit and the stored
path is THE path -- ties, which these inputs are full of, are decided by the reference's `>=` alone.  Stored: int8 codes and int64 paths only."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import alignment_cases as AC  # noqa: E402


def main(reference):
    class _T:
        def __getitem__(self, k):
            return self

        def __call__(self, *a, **k):
            return self
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (lambda f: f)
    for n in ("float64", "float32", "int8", "int32", "int64", "boolean"):
        setattr(nb, n, _T())
    sys.modules["numba"] = nb
    sys.path.insert(0, reference)
    from jatts.modules.alignments import _monotonic_alignment_search

    out = {"shapes": np.array(AC.MAS_FIXTURE_SHAPES, dtype=np.int64)}
    for kind in AC.MAS_EXACT:      # one flat array per kind, the shapes in table order (a zip member per case would cost more than its data)
        codes, paths = [], []
        for tm, ti in AC.MAS_FIXTURE_SHAPES:
            c, lp = AC.mas_input(kind, tm, ti)
            codes.append(c.reshape(-1))
            paths.append(np.asarray(_monotonic_alignment_search(lp)).astype(np.int64))
        out[kind + "_codes"], out[kind + "_paths"] = np.concatenate(codes), np.concatenate(paths)
    path = os.path.join(HERE, "mas_ties.npz")
    np.savez_compressed(path, **out)
    print("mas_ties.npz", os.path.getsize(path), "bytes,", len(AC.MAS_EXACT) * len(AC.MAS_FIXTURE_SHAPES), "cases")


if __name__ == "__main__":
    main(sys.argv[1])
