#!/usr/bin/env python
"""Generate tests/golden/concordance_fns.npz by running the REFERENCE's own concordance functions.  Build container
only (needs the reference checkout, given as the argument):

    python tests/golden/make_concordance_golden.py REFERENCE_CHECKOUT

What is executed, unmodified: tetrad/src/concordance.py of the reference, loaded by file path.  It imports toytree,
loguru and tetrad.src.schema at the top, none of which is needed by the three functions used here; they are stubbed
in sys.modules with empty modules before the load.
  * `qc` (:37-57) and `qd` (:60-71) over a grid of (conc, disc1, disc2), zeros included;
  * `iter_resolved_quartets_table` (:74-94) over a small quartets TSV written here in the reference's format
    ("%.6f" scores), including a row whose scores have different numbers of integer digits (850.2 / 1200.5 /
    1300.1: the reference sorts the score strings, :82) and a row with zero scores.

What is stored: inputs and the reference's outputs.  Data only -- no reference source text.
"""
from __future__ import annotations

import importlib.util
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent


def load_reference(ref: Path):
    for name in ("toytree", "loguru", "tetrad", "tetrad.src", "tetrad.src.schema"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["loguru"].logger = None
    sys.modules["tetrad.src.schema"].Project = object
    sys.modules["toytree"].ToyTree = object
    spec = importlib.util.spec_from_file_location("ref_concordance", ref / "tetrad" / "src" / "concordance.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = Path(sys.argv[1])
    rc = load_reference(ref)
    grid = np.array([(a, b, c) for a in (0, 1, 2, 7, 30) for b in (0, 1, 3, 30) for c in (0, 1, 2, 30)], np.int64)
    node = types.SimpleNamespace
    qc = np.array([rc.qc(node(conc=int(a), disc1=int(b), disc2=int(c))) for a, b, c in grid], np.float64)
    qd = np.array([rc.qd(node(conc=int(a), disc1=int(b), disc2=int(c))) for a, b, c in grid], np.float64)

    rng = np.random.default_rng(7)
    n = 40
    quartets = np.sort(rng.choice(12, size=(n, 4), replace=True), axis=1).astype(np.uint32)
    for i in range(n):                                # distinct sorted taxa
        quartets[i] = np.sort(rng.choice(12, 4, replace=False))
    scores = rng.uniform(0.0, 50.0, size=(n, 3))
    scores[3] = (850.2, 1200.5, 1300.1)              # different numbers of integer digits
    scores[4] = (0.0, 0.0, 0.0)
    scores[5] = (1 / 128, 3 / 128, 5 / 128)          # 6-decimal rounding ties
    topo = rng.integers(0, 3, n).astype(np.uint32)
    nsnps = rng.integers(0, 400, n).astype(np.uint32)
    with tempfile.TemporaryDirectory() as d:
        tsv = Path(d) / "q.tsv"
        with open(tsv, "w") as f:
            for i in range(n):
                f.write("\t".join([*(str(int(x)) for x in quartets[i]), *("%.6f" % x for x in scores[i]),
                                   str(int(topo[i])), str(int(nsnps[i]))]) + "\n")
        text = tsv.read_text()
        rows = list(rc.iter_resolved_quartets_table(tsv))
    ref_q = np.array([r[0] for r in rows], np.uint32)
    ref_topo = np.array([r[1] for r in rows], np.uint32)
    ref_vals = np.array([r[2] for r in rows], np.float64)            # nsnps, weight, score
    np.savez_compressed(OUT / "concordance_fns.npz", grid=grid, qc=qc, qd=qd, tsv=np.frombuffer(text.encode(), np.uint8),
                        quartets=quartets, scores=scores, topo=topo, nsnps=nsnps, ref_quartets=ref_q, ref_topo=ref_topo,
                        ref_values=ref_vals)
    print("wrote", OUT / "concordance_fns.npz", "row 3 (reference):", ref_vals[3])


if __name__ == "__main__":
    main()
