"""ncbi.bidirectional_blast with a Context (the alignments on csrc/sw.hip) against the host model and the recorded reports."""
import os

import numpy as np
import pytest

from pangenomix_amd import _native, ncbi, synth

pytestmark = pytest.mark.gpu


def reports(paths):
    return tuple(open(p).read() for p in paths)


def test_the_recorded_reports_on_the_device(gpu_ctx, golden_dir, tmp_path):
    src = os.path.join(golden_dir, 'blast')
    a, b = os.path.join(src, 'a.faa'), os.path.join(src, 'b.faa')
    ncbi.NCBI_PATH_COUNTS.clear()
    device = reports(ncbi.bidirectional_blast(a, b, str(tmp_path / 'device'), ctx=gpu_ctx))
    assert ncbi.NCBI_PATH_COUNTS['device'] > 0 and ncbi.NCBI_PATH_COUNTS['host'] == 0
    pairs = ncbi.NCBI_PATH_COUNTS['device']
    host = reports(ncbi.bidirectional_blast(a, b, str(tmp_path / 'host'), ctx=None))
    assert ncbi.NCBI_PATH_COUNTS['host'] == pairs and ncbi.NCBI_PATH_COUNTS['device'] == pairs
    assert device == host
    assert device == (open(os.path.join(src, 'a_to_b.tsv')).read(), open(os.path.join(src, 'b_to_a.tsv')).read())


def test_a_protein_over_the_length_limit_goes_to_the_host(gpu_ctx, tmp_path):
    """Word size 6 keeps the chance pairs of the long protein few: the host model aligns every one of them."""
    limit = int(_native.lib().pgx_sw_max_length())
    rng = np.random.default_rng(9)
    base = [synth.AA20[rng.integers(0, 20, int(n))].tobytes() for n in rng.integers(50, 90, 6)]
    names, seqs, _ = synth.related_protein_set(base, seed=3, absent=0.0)
    long_one = base[0] + b'G' * (limit + 1 - len(base[0]))
    a = synth.write_protein_fasta(str(tmp_path / 'a.faa'), ['a%d' % i for i in range(6)] + ['a_long'], base + [long_one])
    b = synth.write_protein_fasta(str(tmp_path / 'b.faa'), names, seqs)
    params = {'evalue': 1e-10, 'word_size': 6}
    ncbi.NCBI_PATH_COUNTS.clear()
    device = reports(ncbi.bidirectional_blast(a, b, str(tmp_path / 'device'), blast_params=params, ctx=gpu_ctx))
    assert ncbi.NCBI_PATH_COUNTS['device'] >= 6 and 1 <= ncbi.NCBI_PATH_COUNTS['host'] <= 3
    assert device == reports(ncbi.bidirectional_blast(a, b, str(tmp_path / 'host'), blast_params=params, ctx=None))
    assert sum(line.startswith('a_long\t') for line in device[0].splitlines()) == 1
