"""Novel-allele calls of pangenomix_amd.mlst with a device context (one near_load per scheme, one near_query per genome that
has a locus without an exact call; csrc/near.hip) against the host path and the hand-written fixtures tests/golden/mlst_novel
and tests/golden/mlst, and one synthetic scheme of 7 x 300 alleles."""
import os

import pytest

import test_mlst_host as exact
import test_mlst_novel_host as host
from pangenomix_amd import mlst, pangenome_analysis as pa, synth

pytestmark = pytest.mark.gpu


def test_fixtures_on_the_device_equal_host_and_recorded_files(golden_dir, gpu_ctx, tmp_path):
    root, scheme_dir, genomes = host.fixture(golden_dir)
    scheme = mlst.load_scheme(scheme_dir)
    mlst.MLST_PATH_COUNTS.clear()
    frame, hits = mlst.call_alleles(scheme, genomes, ctx=gpu_ctx, return_hits=True, min_identity=95)
    assert mlst.MLST_PATH_COUNTS == {'device': 4}
    host_frame, host_hits = mlst.call_alleles(scheme, genomes, return_hits=True, min_identity=95)
    assert frame.equals(host_frame) and hits.equals(host_hits)
    assert host.lines_of(frame, scheme) == host.expected_lines(root)
    host.assert_hits_equal(hits, host.expected_hits(root))
    pa.run_mlst(genomes, str(tmp_path / 'out.tsv'), scheme_dir=scheme_dir, ctx=gpu_ctx, minid=95)
    assert open(tmp_path / 'out.tsv').read() == host.expected_lines(root)
    # the six genomes of the exact fixture: g6's abcA becomes ~1
    root, scheme_dir, genomes, lines, want_hits = host.old_fixture_expectations(golden_dir)
    mlst.MLST_PATH_COUNTS.clear()
    frame, hits = mlst.call_alleles(scheme, genomes, ctx=gpu_ctx, return_hits=True, min_identity=95)
    assert mlst.MLST_PATH_COUNTS == {'device': 6}
    assert host.lines_of(frame, scheme) == lines
    host.assert_hits_equal(hits, want_hits)
    # and without the argument the device path is the one it was
    frame, hits = mlst.call_alleles(scheme, genomes, ctx=gpu_ctx, return_hits=True)
    exact.assert_frame_as_recorded(frame, scheme, root)
    exact.assert_hits_as_recorded(hits, root)


def test_synthetic_scheme_device_equals_host(gpu_ctx, tmp_path):
    """7 loci x 300 alleles of 450 bases (m = 22, blocks of 19), a 200 kbp genome in 5 contigs: half the loci on the minus strand,
    one locus absent, one carrying an allele with one base changed; and a genome of a complete profile"""
    scheme = synth.mlst_scheme(n_loci=7, n_alleles=300, length=450, seed=21)
    key, st = next(iter(scheme.profiles.items()))
    carried = {locus: (number, '+-'[i % 2]) for i, (locus, number) in enumerate(zip(scheme.loci, key))}
    whole = synth.mlst_genome(scheme, str(tmp_path / 'whole.fna'), carried, seed=1)
    partial = dict(carried)
    del partial[scheme.loci[2]]
    holed = synth.mlst_genome(scheme, str(tmp_path / 'holed.fna'), partial, seed=2, novel=(scheme.loci[4],))
    mlst.MLST_PATH_COUNTS.clear()
    frame, hits = mlst.call_alleles(scheme, [whole, holed], ctx=gpu_ctx, return_hits=True, min_identity=95)
    assert mlst.MLST_PATH_COUNTS == {'device': 2}
    host_frame, host_hits = mlst.call_alleles(scheme, [whole, holed], return_hits=True, min_identity=95)
    assert frame.equals(host_frame) and hits.equals(host_hits)
    assert frame['ST'].tolist() == [st, '-']
    assert frame.iloc[0, 3:].tolist() == [str(n) for n in key]
    calls = frame.iloc[1, 3:].tolist()
    assert [c for i, c in enumerate(calls) if i not in (2, 4)] == [str(n) for i, n in enumerate(key) if i not in (2, 4)]
    assert calls[2] == '-' and calls[4].startswith('~')                          # the absent locus; the novel one
    novel = hits[(hits['genome'] == holed) & (hits['locus'] == scheme.loci[4])]
    assert len(novel) == 1
    row = novel.iloc[0]
    assert (row['mismatches'], row['copies'], row['strand']) == (1, 0, carried[scheme.loci[4]][1])
    # the allele that was planted is one base away; the call is the lowest number among the alleles that are
    planted = dict(scheme.alleles[scheme.loci[4]])[key[4]]
    called = dict(scheme.alleles[scheme.loci[4]])[int(calls[4][1:])]
    assert int(calls[4][1:]) <= key[4] and sum(a != b for a, b in zip(planted, called)) <= 2
    assert (hits[hits['mismatches'] == 0]['copies'] == 1).all() and len(hits) == 7 + 6


def test_a_scheme_with_a_short_block_goes_to_the_host(golden_dir, gpu_ctx):
    """at 80 % the fixture's alleles of 40 bases may differ in 8: blocks of 4 bases, under the 8 the device path asks for"""
    root, scheme_dir, genomes = host.fixture(golden_dir)
    scheme = mlst.load_scheme(scheme_dir)
    assert mlst.max_mismatches(40, 80) == 8
    mlst.MLST_PATH_COUNTS.clear()
    frame, hits = mlst.call_alleles(scheme, genomes, ctx=gpu_ctx, return_hits=True, min_identity=80)
    assert mlst.MLST_PATH_COUNTS == {'host': 4}
    host_frame, host_hits = mlst.call_alleles(scheme, genomes, return_hits=True, min_identity=80)
    assert frame.equals(host_frame) and hits.equals(host_hits)
    assert frame['abcA'].tolist()[:2] == ['~3', '~3']
