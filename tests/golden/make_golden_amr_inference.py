"""Writes tests/golden/amr_inference: a generated AMR table in PATRIC's column layout (table.tsv) and what the reference's
extract_primary_stnds, extract_mic_calls, extract_mic_sir_mappings, validate_mic_sir_mappings and infer_sir
(amr_inference.py) returned and printed on it (expected.json). Needs the reference checkout -- its directory is the first
argument or $PANGENOMIX_REFERENCE; nothing of it is written or copied.

The reference's amr_inference.py does not parse as Python 3 (five `print` statements), and its extract_primary_stnds takes
len() of a filter(). This script reads the file's text, translates it in memory with lib2to3 and the two fixers fix_print
and fix_filter -- which change exactly those five lines and that one -- and executes the result as a module.

The table holds two organisms and a genome of neither; a combination drug with 'a/b' MICs; polymyxin_b and nalidixic_acid
(underscores, no combinations); a drug under min_entries; the standard 'missing', a second standard and rows without one;
methods and units that give no MIC; every sign (`measurement` carries an inequality, `measurement_value` does not, and both
are read as strings); the MIC '4' beside '4.0'; S, I and R ranges that overlap, so that the order
of the classes decides; a MIC mapped to two classes and a case whose susceptible MICs reach above its resistant ones, for
the validator's prints. It is built so that the translated reference runs: in the rows that are counted, no null meets a
string where tuples are sorted -- resistant_phenotype and the column at position -5 (testing_standard here) hold no null
there, and the sign of a MIC is either always exact (null, '=', '==') or always the same inequality.
Nothing recorded depends on the order in which a set of strings iterates: df_primary_stnds is recorded by sorted index,
and the order of the classes in mic_ranges is recorded and handed on by the tests."""
import contextlib
import io
import json
import os
import sys
import types
from lib2to3 import refactor

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ['PANGENOMIX_REFERENCE']
OUT = os.path.join(HERE, 'amr_inference')

COLUMNS = ['genome_id', 'genome_name', 'taxon_id', 'antibiotic', 'resistant_phenotype', 'measurement', 'measurement_sign',
           'measurement_value', 'measurement_unit', 'laboratory_typing_method', 'laboratory_typing_method_version',
           'laboratory_typing_platform', 'vendor', 'testing_standard', 'testing_standard_year', 'computational_method',
           'computational_method_version', 'source']
ORG_TO_GIDS = {'Klebsiella pneumoniae': ['573.1', '573.2', '573.3', '573.4'],
               'Escherichia coli': ['562.1', '562.2', '562.3', '562.4', '562.5', '562.6']}
MIN_ENTRIES, MINIMUM_CALLS = 30, 3
EXACT_SIGNS = (None, '=', '==', None)
BOUND_SIGNS = {'0.125': '<', '0.25': '<=', '32': '>=', '64': '>', '0.5/9.5': '<=', '32/608': '>'}

# (organism, drug): [(mic, sir, standard, rows)]
CALLS = {
    ('Escherichia coli', 'ampicillin'): [
        ('0.125', 'susceptible', 'clsi', 3), ('0.25', 'susceptible', 'clsi', 4), ('1', 'susceptible', 'clsi', 5),
        ('2', 'susceptible', 'clsi', 6), ('4', 'susceptible', 'clsi', 4), ('4.0', 'intermediate', 'clsi', 3),
        ('8', 'intermediate', 'clsi', 5), ('8', 'resistant', 'clsi', 3), ('16', 'resistant', 'clsi', 6),
        ('32', 'resistant', 'clsi', 4), ('64', 'resistant', 'clsi', 3), ('2', 'intermediate', 'clsi', 2),
        ('2', 'susceptible', 'eucast', 7), ('16', 'resistant', 'eucast', 5), ('4', 'susceptible', 'missing', 4),
        ('1', 'not defined', 'clsi', 3)],
    ('Escherichia coli', 'amoxicillin_clavulanic_acid'): [
        ('0.5/9.5', 'susceptible', 'clsi', 3), ('2/1', 'susceptible', 'clsi', 5), ('4/2', 'susceptible', 'clsi', 4),
        ('8/4', 'intermediate', 'clsi', 3), ('16/8', 'resistant', 'clsi', 6), ('32/608', 'resistant', 'clsi', 3),
        ('2/1', 'susceptible', 'eucast', 6), ('16/8', 'resistant', 'missing', 3)],
    ('Escherichia coli', 'polymyxin_b'): [
        ('0.5', 'susceptible', 'eucast', 9), ('1', 'susceptible', 'eucast', 8), ('2', 'susceptible', 'eucast', 5),
        ('4', 'resistant', 'eucast', 6), ('8', 'resistant', 'eucast', 4), ('1', 'susceptible', 'clsi', 9)],
    ('Escherichia coli', 'rare_drug'): [('1', 'susceptible', 'clsi', 5), ('4', 'resistant', 'clsi', 4)],
    ('Klebsiella pneumoniae', 'nalidixic_acid'): [
        ('2', 'susceptible', 'clsi', 8), ('4', 'susceptible', 'clsi', 6), ('16', 'resistant', 'clsi', 7),
        ('32', 'resistant', 'clsi', 5), ('8', 'intermediate', 'eucast', 8), ('4', 'susceptible', 'eucast', 9)],
    ('Klebsiella pneumoniae', 'ciprofloxacin'): [
        ('0.25', 'susceptible', 'clsi', 5), ('0.5', 'susceptible', 'clsi', 6), ('16', 'susceptible', 'clsi', 3),
        ('1', 'intermediate', 'clsi', 4), ('2', 'resistant', 'clsi', 6), ('4', 'resistant', 'clsi', 5),
        ('0.5', 'susceptible', 'bsac', 6), ('4', 'resistant', 'bsac', 6)],
    ('Klebsiella pneumoniae', 'ampicillin'): [('32', 'resistant', 'clsi', 6), ('16', 'resistant', 'clsi', 5)],
}
METHODS = ('broth_microdilution', 'etest', 'vitek_2', 'agar_dilution')


def table():
    rows, k = [], 0

    def add(org, drug, sir, mic, sign, unit, method, standard, gid=None):
        gids = ORG_TO_GIDS[org]
        # PATRIC's `measurement` carries the inequality, `measurement_value` does not
        measurement = (sign if sign in ('<', '<=', '>', '>=') else '') + mic if mic is not None else None
        rows.append([gid or gids[len(rows) % len(gids)], org + ' strain', gids[0].split('.')[0], drug, sir, measurement, sign, mic,
                     unit, method, None, None, None, standard, 2015 if standard else None, None, None, 'fixture'])

    for (org, drug), calls in CALLS.items():
        for mic, sir, standard, n in calls:
            for _ in range(n):
                sign = BOUND_SIGNS.get(mic, EXACT_SIGNS[k % 4])
                add(org, drug, sir, mic, sign, 'mg/L', METHODS[k % 4], standard)
                k += 1
        # what gives no MIC call but counts as a row of the case: a disk diffusion, a MIC method in mm, a computed phenotype
        # without a measurement (and without a standard), a phenotype that is missing altogether
        for j in range(4):
            add(org, drug, 'resistant' if j % 2 else 'susceptible', '%d' % (12 + j), None, 'mm', 'disk_diffusion', 'clsi')
        add(org, drug, 'susceptible', '21', None, 'mm', 'etest', 'clsi')
        add(org, drug, 'resistant', '2', '=', 'mg/L', 'computational prediction', 'clsi')
        for j in range(3):
            add(org, drug, 'resistant', None, None, None, None, None)
        add(org, drug, None, None, None, None, 'disk_diffusion', None)
    add('Escherichia coli', 'ampicillin', 'resistant', '64', '>', 'mg/L', 'etest', 'clsi', gid='999.1')
    add('Escherichia coli', 'ampicillin', 'susceptible', '1', None, 'mg/L', 'etest', 'clsi', gid='999.1')
    # asked of infer_sir only: MICs that were never observed, inside, between and outside the ranges, with every sign
    for mic, sign in (('3', None), ('3', '='), ('6', '=='), ('0.06', '<'), ('0.06', '<='), ('128', '>'), ('128', '>='),
                      ('128', None), ('0.06', None), ('3', '<'), ('3', '>'), ('4.0', None), ('4', None), ('4.00', None)):
        add('Escherichia coli', 'ampicillin', 'resistant', mic, sign, 'mm', 'etest', 'clsi')
        add('Klebsiella pneumoniae', 'ciprofloxacin', 'resistant', mic, sign, 'mm', 'etest', 'clsi')
    add('Escherichia coli', 'amoxicillin_clavulanic_acid', 'resistant', '3', None, 'mm', 'etest', 'clsi')
    add('Escherichia coli', 'amoxicillin_clavulanic_acid', 'resistant', '64/32', None, 'mm', 'etest', 'clsi')
    return pd.DataFrame(rows, columns=COLUMNS)


def read_table(path):
    """as the tests read it: ids and MICs stay strings"""
    return pd.read_csv(path, sep='\t', dtype={'genome_id': str, 'measurement': str, 'measurement_value': str, 'taxon_id': str})


def translated_reference():
    """the reference's amr_inference as a module of this interpreter, and the lines the translation changed"""
    path = os.path.join(REFERENCE, 'pangenomix', 'amr_inference.py')
    with io.open(path, encoding='utf-8') as f:
        source = f.read()
    if not source.endswith('\n'):
        source += '\n'                                   # (lib2to3's grammar wants the last line ended)
    tool = refactor.RefactoringTool(['lib2to3.fixes.fix_print', 'lib2to3.fixes.fix_filter'])
    translated = str(tool.refactor_string(source, path))
    changed = [i for i, (a, b) in enumerate(zip(source.split('\n'), translated.split('\n'))) if a != b]
    module = types.ModuleType('reference_amr_inference')
    exec(compile(translated, path, 'exec'), module.__dict__)
    return module, changed


def plain(x):
    """JSON values: a null is None, numpy scalars are Python's"""
    if isinstance(x, dict):
        return [[plain(k), plain(v)] for k, v in x.items()]              # (a list keeps the order, and tuples as keys)
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if x is None or (isinstance(x, float) and x != x):
        return None
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    return x


def plain_frame(df):
    return {'index': plain(df.index.tolist()), 'columns': df.columns.tolist(), 'dtypes': [str(t) for t in df.dtypes],
            'data': plain(df.values.tolist())}


def main():
    ref, changed = translated_reference()
    assert len(changed) == 6, changed
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, 'table.tsv')
    table().to_csv(path, sep='\t', index=False)
    df_amr = read_table(path)

    df_stnds = ref.extract_primary_stnds(ORG_TO_GIDS, df_amr, MIN_ENTRIES)
    df_calls = ref.extract_mic_calls(ORG_TO_GIDS, df_amr, MIN_ENTRIES)
    case_to_standard = df_stnds.top_stnd
    sir_order = list(ref.extract_mic_sir_mappings.__defaults__[1])        # the order this process iterates the set in
    mic_ref_calls, mic_ranges = ref.extract_mic_sir_mappings(df_calls, case_to_standard, MINIMUM_CALLS)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        ref.validate_mic_sir_mappings(mic_ref_calls, mic_ranges)
    org_of = {gid: org for org, gids in ORG_TO_GIDS.items() for gid in gids}
    asked = df_amr[df_amr.genome_id.map(lambda g: g in org_of) & pd.notnull(df_amr.measurement)]
    inferred = [ref.infer_sir(org_of[gid], drug, mic, sign, mic_ranges, case_to_standard)
                for gid, drug, mic, sign in zip(asked.genome_id, asked.antibiotic, asked.measurement_value, asked.measurement_sign)]
    expected = {
        'org_to_gids': ORG_TO_GIDS, 'min_entries': MIN_ENTRIES, 'minimum_calls': MINIMUM_CALLS,
        'primary_stnds': plain_frame(df_stnds.sort_index()),
        'mic_calls': plain_frame(df_calls),
        'sir_order': sir_order,
        'mic_ref_calls': plain(mic_ref_calls),
        'mic_ranges': plain(mic_ranges),
        'validate_printed': printed.getvalue(),
        'asked_rows': asked.index.tolist(),
        'inferred': plain(inferred),
    }
    with open(os.path.join(OUT, 'expected.json'), 'w') as f:
        json.dump(expected, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s: %d rows, %d cases, %d calls, %d classes hit' % (OUT, len(df_amr), len(df_stnds), len(df_calls),
                                                                    sum(1 for s, _ in inferred if isinstance(s, str))))
    print(printed.getvalue())


if __name__ == '__main__':
    main()
