"""Writes tests/golden/blast: a.faa (twelve proteins), b.faa (derived from it by synth.related_protein_set, plus the
known-answer cases of tests/test_ncbi_host.py as proteins of their own) and the two reports of ncbi.bidirectional_blast on the
host model (ctx=None). Run from the repository root: python tests/golden/make_golden_blast.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from pangenomix_amd import ncbi, synth  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'blast')


def main():
    rng = np.random.default_rng(62)
    a = [synth.AA20[rng.integers(0, 20, int(n))].tobytes() for n in rng.integers(70, 160, 12)]
    names_b, b, origin = synth.related_protein_set(a[:10], seed=7, absent=0.2)
    # by hand: a10 comes back unchanged (100.000, no gap), a11 with residues 40..44 deleted (one gap of 5)
    names_b += ['b_same', 'b_del5']
    b += [a[10], a[11][:40] + a[11][45:]]
    os.makedirs(OUT, exist_ok=True)
    synth.write_protein_fasta(os.path.join(OUT, 'a.faa'), ['a%d' % i for i in range(12)], a)
    synth.write_protein_fasta(os.path.join(OUT, 'b.faa'), names_b, b)
    with open(os.path.join(OUT, 'origin.tsv'), 'w') as f:
        for name, k in zip(names_b, list(origin) + [10, 11]):
            f.write('%s\ta%d\n' % (name, k))
    ncbi.bidirectional_blast(os.path.join(OUT, 'a.faa'), os.path.join(OUT, 'b.faa'), OUT)


if __name__ == '__main__':
    main()
