"""weboflife.get_node_gene_content_table on the device against what the reference returned (tests/golden/weboflife) and
against the host path in process. Counts are integers and the division is the host's on both paths: frames are equal bit
for bit."""
import warnings

import numpy as np
import pandas as pd
import pytest

import weboflife_cases as cases
from pangenomix_amd import synth
from pangenomix_amd import weboflife as wol
from weboflife_cases import as_frame, check_irregular, counts, lsdf, path_of

pytestmark = pytest.mark.gpu
EXPECTED = cases.expected()


@pytest.mark.parametrize('kind', ('frame', 'lsdf'))
def test_table_on_the_device_is_the_references(kind, gpu_ctx):
    G = cases.graph(wol.PhyloGraph, cases.edges())
    frame = cases.table()
    before = counts()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = wol.get_node_gene_content_table(G, frame if kind == 'frame' else lsdf(frame), cases.mapping(), cases.ROOT, ctx=gpu_ctx)
    assert path_of(before) == ['table_device']
    pd.testing.assert_frame_equal(got, as_frame(EXPECTED['content']), check_exact=True)


def test_chunked_device_table_is_the_host_table(gpu_ctx, monkeypatch):
    G, root, m, tab = synth.phylogeny(300, 3, n_genes=700, max_children=5, mapped_internal=12, unmapped_leaves=15, unused_species=4)
    want = wol.get_node_gene_content_table(G, tab, m, root)
    monkeypatch.setattr(wol, '_CHUNK_BYTES', 4 * len(G) * 256)          # 256 genes per call: three calls, the last one short
    assert wol._chunk_genes(len(G)) == 256
    before = counts()
    got = wol.get_node_gene_content_table(G, tab, m, root, ctx=gpu_ctx)
    assert path_of(before) == ['table_device']
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    assert np.isnan(got.to_numpy()).any() and (got.loc[root] > 0).any()
    some = list(tab.index[[699, 3, 256, 255]])
    pd.testing.assert_frame_equal(wol.get_node_gene_content_table(G, tab, m, root, genes=some, ctx=gpu_ctx), want[some], check_exact=True)


@pytest.mark.parametrize('name', cases.IRREGULAR)
def test_irregular_input_gives_what_the_host_gives(name, gpu_ctx):
    check_irregular(name, gpu_ctx, 'table_device' if name == 'shared_child_of_mapped' else 'table_host')
