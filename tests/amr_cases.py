"""What tests/test_amr_host.py and tests/test_gpu_amr.py share: the recorded case of tests/golden/amr (written by
tests/golden/make_golden_amr.py from the reference's amr.py), read once, and the calls that run pangenomix_amd.amr on it with
or without a device context."""
import ast
import json
import os

import pandas as pd

from pangenomix_amd import amr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'amr')
OBO, RGI, ANNOTATIONS = (os.path.join(GOLDEN, name) for name in ('aro.obo', 'rgi.txt', 'annotations.tsv'))
with open(os.path.join(GOLDEN, 'expected.json')) as _f:
    EXPECTED = json.load(_f)
DRUGS, PROBABLE_ARGS = EXPECTED['drugs'], EXPECTED['probable_args']


def recorded_frame(name):
    """a frame as the generator's to_csv wrote it; AROs and hits stay strings"""
    return pd.read_csv(os.path.join(GOLDEN, name), sep='\t', index_col=0, dtype={'card_hits': str, 'related_aros': str})


def graph(use_networkx=None):
    old = amr.USE_NETWORKX
    amr.USE_NETWORKX = use_networkx
    try:
        return amr.construct_aro_to_drug_network(OBO)
    finally:
        amr.USE_NETWORKX = old


def resistome(capsys, G, ctx=None, rgi=RGI, drugs=None, **kwargs):
    """((df_rgi, df_aro), printed)"""
    capsys.readouterr()
    result = amr.build_resistome(rgi, DRUGS if drugs is None else drugs, G, ctx=ctx, **kwargs)
    return result, capsys.readouterr().out


def probable(capsys, df_aro, G, aro_names, ctx=None, annotations=ANNOTATIONS, **kwargs):
    """(df_prob, the printed search terms as a dict of sets, printed)"""
    args = dict(PROBABLE_ARGS, G_aro=G, aro_names=aro_names)
    args.update(kwargs)
    capsys.readouterr()
    df_prob = amr.generate_probable_hits_from_annotations(df_aro, annotations, ctx=ctx, **args)
    printed = capsys.readouterr().out
    return df_prob, ast.literal_eval(printed.strip()) if printed.strip() else None, printed


def assert_prob_equal(got, want):
    """the same rows under the same index values (pandas' unstable sort by drug may order equal drugs differently)"""
    pd.testing.assert_frame_equal(got.sort_index(), want.sort_index())
    assert got['drug'].tolist() == sorted(got['drug'].tolist())
