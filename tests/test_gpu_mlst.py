"""pangenomix_amd.mlst with a device context (one pattern_load per scheme, one pattern_query per genome; csrc/pattern.hip)
against the host path and the hand-written fixture tests/golden/mlst, and one synthetic scheme of 7 x 300 alleles."""
import os

import pytest

import test_mlst_host as host
from pangenomix_amd import mlst, pangenome_analysis as pa, synth

pytestmark = pytest.mark.gpu


def test_fixture_on_the_device_equals_host_and_recorded_files(golden_dir, gpu_ctx, tmp_path):
    root, scheme_dir, genomes = host.fixture(golden_dir)
    scheme = mlst.load_scheme(scheme_dir)
    mlst.MLST_PATH_COUNTS.clear()
    frame, hits = mlst.call_alleles(scheme, genomes, ctx=gpu_ctx, return_hits=True)
    assert mlst.MLST_PATH_COUNTS == {'device': 6}
    host_frame, host_hits = mlst.call_alleles(scheme, genomes, return_hits=True)
    assert frame.equals(host_frame) and hits.equals(host_hits)
    host.assert_frame_as_recorded(frame, scheme, root)
    host.assert_hits_as_recorded(hits, root)
    pa.run_mlst(os.path.join(root, 'genomes'), str(tmp_path / 'out.tsv'), scheme_dir=scheme_dir, ctx=gpu_ctx)
    assert open(tmp_path / 'out.tsv').read() == host.expected_lines(root)


def test_a_genome_that_is_not_ascii_is_scanned_on_the_host(golden_dir, gpu_ctx, tmp_path):
    root, scheme_dir, genomes = host.fixture(golden_dir)
    scheme = mlst.load_scheme(scheme_dir)
    data = open(genomes[0], 'rb').read()
    odd = tmp_path / 'odd.fna'
    odd.write_bytes(data + b'>extra\nACGT\xc3\xa9ACGT\n')
    mlst.MLST_PATH_COUNTS.clear()
    frame = mlst.call_alleles(scheme, [genomes[1], str(odd)], ctx=gpu_ctx)
    assert mlst.MLST_PATH_COUNTS == {'device': 1, 'host': 1}
    assert frame['ST'].tolist() == ['2', '1'] and frame['abcA'].tolist() == ['2', '1']


def test_synthetic_scheme_device_equals_host(gpu_ctx, tmp_path):
    """7 loci x 300 alleles of 450 bases, a 200 kbp genome in 5 contigs: half the loci on the minus strand, one locus absent,
    one carrying an allele the scheme does not hold; and a genome of a complete profile"""
    scheme = synth.mlst_scheme(n_loci=7, n_alleles=300, length=450, seed=21)
    key, st = next(iter(scheme.profiles.items()))
    carried = {locus: (number, '+-'[i % 2]) for i, (locus, number) in enumerate(zip(scheme.loci, key))}
    whole = synth.mlst_genome(scheme, str(tmp_path / 'whole.fna'), carried, seed=1)
    partial = dict(carried)
    del partial[scheme.loci[2]]
    holed = synth.mlst_genome(scheme, str(tmp_path / 'holed.fna'), partial, seed=2, novel=(scheme.loci[4],))
    mlst.MLST_PATH_COUNTS.clear()
    frame, hits = mlst.call_alleles(scheme, [whole, holed], ctx=gpu_ctx, return_hits=True)
    assert mlst.MLST_PATH_COUNTS == {'device': 2}
    host_frame, host_hits = mlst.call_alleles(scheme, [whole, holed], return_hits=True)
    assert frame.equals(host_frame) and hits.equals(host_hits)
    assert frame['ST'].tolist() == [st, '-']
    assert frame.iloc[0, 3:].tolist() == [str(n) for n in key]
    assert frame.iloc[1, 3:].tolist() == [str(n) if i not in (2, 4) else '-' for i, n in enumerate(key)]
    assert hits['strand'].tolist() == ['+', '-', '+', '-', '+', '-', '+'] + ['+', '-', '-', '-', '+']
    assert (hits['copies'] == 1).all() and len(set(hits['contig'])) == 5
