#!/usr/bin/env python
"""Golden scores for compute_concept_list_similarity (reference fcd.py:168-196), produced by RUNNING THE REFERENCE in the
build container (needs /root/reference; it never travels to the GPU box):

    python tests/golden/make_golden_fcd_similarity.py

As in make_golden_fcd.py, an empty placeholder module is registered under the name seaborn first; nothing of it is
called. The cases are those of tests/fcd_similarity_model.py (CASES / case_inputs): 45 pairs of the concept lists in
tests/golden/fcd/*.npz on their own table, and concept lists generated from a seed. Only the scores are stored:
tests/golden/fcd_similarity/scores.json maps the case name to float.hex() of the reference's score, or to the class
name of the exception the reference raised (an all-zero table: ZeroDivisionError).
"""
import json
import os
import sys
import types
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, '/root/reference')
sys.modules.setdefault('seaborn', types.ModuleType('seaborn'))

import pangenomix.fcd as ref_fcd              # noqa: E402
import fcd_similarity_model as sim            # noqa: E402


def main():
    out = {}
    for name in sim.CASES:
        F1, F2, S = sim.case_inputs(name)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            try:
                out[name] = float(ref_fcd.compute_concept_list_similarity(F1, F2, S)).hex()
            except Exception as e:             # noqa: BLE001 (the exception is the expectation)
                out[name] = type(e).__name__
        print(name, out[name])
    os.makedirs(os.path.dirname(sim.SCORES), exist_ok=True)
    with open(sim.SCORES, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
