"""Records tests/golden/sa_cell_diet.npz: the outputs of pasnl_sa_cell / pasnl_sa_cell_pre (both centre forms) for the cases of
tests/sa_cell_diet_cases.py, as the library of the checked-out commit computes them on an MI355X.

It was run on the commit before the cells' load order, wait counts and skip-fold placement changed (no arithmetic did);
tests/test_gpu_sa_cell_diet.py holds every later build to those bits.  Run it again only on a commit whose cell arithmetic is
meant to become the new reference:

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_sa_cell_diet.py [out.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import sa_cell_diet_cases as C  # noqa: E402
from guarded import NAN_BYTE  # noqa: E402


def main(path):
    from pointasnl_amd import _hip

    _hip.lib()
    _hip.require_device()
    rec = {}
    for case in C.CASES:
        d = C.inputs(case)
        for centre0 in (False, True):
            r = C.run(case, d, centre0, NAN_BYTE)
            assert r.guards, (case, centre0)
            for name, a in C.record(case, r, centre0).items():
                rec[f"{C.case_id(case)}/{'centre0' if centre0 else 'table'}/{name}"] = a
    np.savez(path, **rec)
    print(f"{path}: {len(rec)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sa_cell_diet.npz"))
