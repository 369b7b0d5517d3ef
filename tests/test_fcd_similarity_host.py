"""Comparing two concept lists, what can be checked without a GPU: the numpy model of the device's rule
(tests/fcd_similarity_model.py) and the untouched host loop of pangenomix_amd/fcd.py both give the scores the reference
itself produced (tests/golden/fcd_similarity/scores.json, written by make_golden_fcd_similarity.py), bit for bit, so the
model is a fair yardstick for the pairing and the matrix, which the reference throws away. Every comparison is exact."""
import inspect
import json

import numpy as np
import pytest

import fcd_similarity_model as sim
from pangenomix_amd import fcd

SCORES = json.load(open(sim.SCORES))


def test_the_recorded_cases_are_the_cases():
    assert sorted(SCORES) == sorted(sim.CASES) and len(sim.CASES) == 45 + len(sim.GENERATED)
    assert SCORES['all_zeros__all_zeros'] == 'ZeroDivisionError'
    assert SCORES['limit_0__limit_0'] == (0.0).hex()
    assert max(float.fromhex(v) for v in SCORES.values() if v.startswith('0x')) > 1.0      # overlapping concepts


@pytest.mark.parametrize('name', sim.CASES)
def test_model_and_host_loop_reproduce_the_reference(name):
    F1, F2, S = sim.case_inputs(name)
    want = sim.expected(name)
    if not SCORES[name].startswith('0x'):
        assert SCORES[name] == 'ZeroDivisionError'
        with pytest.raises(ZeroDivisionError):
            fcd.compute_concept_list_similarity(F1, F2, S)
        with pytest.raises(ZeroDivisionError):
            want['total'] / float(np.sum(S))
    else:
        assert fcd.compute_concept_list_similarity(F1, F2, S).hex() == SCORES[name]
        assert (want['total'] / float(np.sum(S))).hex() == SCORES[name]
    # the host loop's own total: the same call over a table with a single one
    assert fcd.compute_concept_list_similarity(F1, F2, np.ones((1, 1), dtype=int)) == float(want['total'])
    assert want['total'] < 2 ** 53
    assert want['match'].size == min(len(F1), len(F2)) and np.unique(want['match']).size == want['match'].size


def test_disjoint_families_pair_in_order():
    name = [n for n in sim.CASES if n.endswith('_disjoint')][0]
    want = sim.expected(name)
    assert not want['O'].any() and want['total'] == 0
    assert want['match'].tolist() == list(range(want['match'].size))


def test_the_generated_families_hold_their_edge_cases():
    F1, F2, _ = sim.case_inputs('gen_70001x65_257x130')
    for F in (F1, F2):
        assert len(set(F[0][0])) < len(F[0][0]) and len(set(F[0][1])) < len(F[0][1])
        assert F[1][0] == [] and F[2][1] == [] and F[3] == F[4]
    O = sim.expected('gen_70001x65_257x130')['O']
    assert np.array_equal(O[:, 3], O[:, 4]) and O[:, 3].any()                             # exact ties


F3 = [((0, 2), (1,)), ((1, 2, 3), (0, 2)), ((3,), (3, 1))]


def test_the_ctx_keyword_defaults_to_the_host_loop():
    sig = inspect.signature(fcd.compute_concept_list_similarity)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ('F1', inspect.Parameter.empty), ('F2', inspect.Parameter.empty), ('S', inspect.Parameter.empty), ('ctx', None)]
    S = np.ones((4, 4), dtype=int)
    assert fcd.compute_concept_list_similarity(F3, F3, S, ctx=None) == fcd.compute_concept_list_similarity(F3, F3, S)
    assert fcd.compute_concept_list_similarity(F3, F3, S, ctx=None) == (2 + 6 + 2) / 16.0


def test_indices_outside_the_table_are_refused_before_any_device_call():
    for bad in ([((4,), (0,))], [((0,), (4,))], [((-1,), (0,))]):
        with pytest.raises(IndexError):
            fcd.match_concept_lists(bad, F3, (4, 4))
        with pytest.raises(IndexError):
            fcd.concept_overlaps(F3, bad, (4, 4))
