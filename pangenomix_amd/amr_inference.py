"""SIR phenotypes from MICs (reference amr_inference.py): the most common testing standard of every organism x drug case of
a PATRIC AMR table, its distinct MIC calls, the MIC -> SIR mappings they give and the inference itself. The reference's
names, positional order, defaults and module constants; `ctx=None` is the reference restated -- with its quirks, and with
the meaning its Python 2 statements had where Python 3 raises -- and a _native.Context gives the device path:

    extract_primary_stnds    pgx_tuple_group over (organism, drug) and over (organism, drug, standard)
    extract_mic_calls        pgx_tuple_group over (organism, drug) and over the seven columns of a MIC call
    infer_sir_batch          one pgx_mic_infer over all rows (new: infer_sir itself is a scalar function)

The device path takes regular input only and leaves anything else to the host code unchanged; AMR_INFERENCE_PATH_COUNTS
says which path ran. It reaches the library through ctx.tuple_group(...) and ctx.mic_infer(...) alone.
infer_sir, extract_mic_sir_mappings, validate_mic_sir_mappings and __is_combination_therapy__ are host code."""
from __future__ import print_function
import collections

import numpy as np
import pandas as pd

NULL_TESTING_STANDARDS = {'missing'}   # testing standard to treat as null
ACCEPTED_MIC_METHODS = {
    'mic', 'broth_microdilution', 'agar_dilution', 'vitek_2',
    'etest', 'agar_dilution_or_etest', 'sensititre', 'bd_phoenix',
    'mic broth microdilution', 'bd_phoenix_and_etest', 'liofilchem'
}   # lab methods on PATRIC that provide MIC values (laboratory_typing_method)
MIC_EQUALITY_SIGNS = {np.nan, '=', '=='}           # MIC equality signs accepted by infer_sir()
MIC_INEQUALITY_SIGNS = {'>', '>=', '<', '<='}      # MIC inequality signs accepted by infer_sir()
MIC_BOUNDING_CASES = [('susceptible', {'<', '<='}), ('resistant', {'>', '>='})]   # MIC bounding for infer_sir()

# primary_stnds_device / primary_stnds_host, mic_calls_device / mic_calls_host, infer_sir_batch_device / _host: per call
AMR_INFERENCE_PATH_COUNTS = collections.Counter()

_TUPLE_MAX_ROWS = 1 << 24              # pgx_tuple_group
_MIC_MAX_ROWS, _MIC_MAX_TABLE = 1 << 31, 1 << 24   # pgx_mic_infer


class _Irregular(Exception):
    """input the device path does not take: the whole call goes to the host code"""


# what the encoding raises on input it was not written for (a missing column, an unhashable value): such input is irregular
# too, and the host code then returns or raises as it does without a context. A library error is none of these.
_ENCODING_ERRORS = (_Irregular, AttributeError, KeyError, IndexError, TypeError, ValueError)


def infer_sir(org, antibiotic, measurement_value, measurement_sign, mic_ranges, df_case_to_standard):
    """(sir, primary_stnd) inferred from a MIC by the previously observed MICs of its organism x drug case (reference
    :27-100), or (np.nan, np.nan). mic_ranges: {(organism, drug, standard): {SIR: [observed MICs]}} of
    extract_mic_sir_mappings; df_case_to_standard: a Series from 'org|drug' to the primary standard (the top_stnd column of
    extract_primary_stnds). An exact MIC (sign np.nan, '=', '==') is tried on the classes in the order mic_ranges[entry]
    iterates: first whether the MIC was observed, then -- unless the drug is a combination or the MIC is not a number --
    whether it lies in the class's range, open below for 'susceptible' and above for 'resistant'. A bounded MIC is tried on
    'susceptible' ('<', '<=') or 'resistant' ('>', '>=') alone. As in the reference: a string MIC is never `in` a list of
    floats, a NaN sign other than the np.nan object is in neither set of signs, and the range test raises TypeError for a
    class that holds a string MIC."""
    try:                                                 # checking for combination therapies
        mic_val = float(measurement_value)
        mic_is_numeric = True
    except ValueError:
        mic_is_numeric = False
    is_likely_combo = __is_combination_therapy__(antibiotic) or not mic_is_numeric

    case = org + '|' + antibiotic
    if case in df_case_to_standard.index:
        primary_stnd = df_case_to_standard[case]
        entry = (org, antibiotic, primary_stnd)
        if entry in mic_ranges:
            case_mic_ranges = mic_ranges[entry]
            if measurement_sign in MIC_EQUALITY_SIGNS:   # exact MIC, check S, I, R
                for sir in case_mic_ranges:
                    if measurement_value in case_mic_ranges[sir]:    # check if MIC was previously observed
                        return sir, primary_stnd
                    elif not is_likely_combo:            # numeric MIC for single therapy, check range
                        sir_min = min(case_mic_ranges[sir])
                        sir_max = max(case_mic_ranges[sir])
                        mic_val = float(measurement_value)
                        if (sir == 'susceptible' or mic_val >= sir_min) and (sir == 'resistant' or mic_val <= sir_max):
                            return sir, primary_stnd
            elif measurement_sign in MIC_INEQUALITY_SIGNS:           # bounded MIC, check S and R only
                for sir, sir_signs in MIC_BOUNDING_CASES:
                    if sir in case_mic_ranges and measurement_sign in sir_signs:
                        if measurement_value in case_mic_ranges[sir]:
                            return sir, primary_stnd
                        elif not is_likely_combo:
                            sir_min = min(case_mic_ranges[sir])
                            sir_max = max(case_mic_ranges[sir])
                            mic_val = float(measurement_value)
                            if (sir == 'susceptible' or mic_val >= sir_min) and (sir == 'resistant' or mic_val <= sir_max):
                                return sir, primary_stnd
    return np.nan, np.nan


def extract_mic_sir_mappings(df_mic_calls, df_case_to_standard, minimum_calls=3,
                             allowed_sirs={'susceptible', 'resistant', 'intermediate'}):
    """(mic_ref_calls, mic_ranges) of the exact MIC calls (extract_mic_calls) seen at least minimum_calls times under their
    case's primary standard (reference :103-170): {(organism, drug, standard): {MIC: {SIR: count}}} with the MICs as
    strings, and {(organism, drug, standard): {SIR: sorted [observed MICs]}} with the MICs as floats except those with a
    slash (combination therapies). The classes of a case come in the order `allowed_sirs` iterates."""
    mic_ref_calls = {}                                   # {(org, drug, stnd): mic: sir: count}
    for org in df_mic_calls.organism.unique():
        df_org_mics = df_mic_calls[df_mic_calls.organism == org]
        df_org_mics = df_org_mics[df_org_mics['count'] >= minimum_calls]     # only use mappings with enough calls
        df_org_mics = df_org_mics[pd.isnull(df_org_mics.mic_sign)]          # only use exact MIC calls
        for drug in df_org_mics.drug.unique():
            case = org + '|' + drug
            if case in df_case_to_standard.index:
                case_stnd = df_case_to_standard[case]
                df_org_drug = df_org_mics[df_org_mics.drug == drug]
                df_org_drug_stnd = df_org_drug[df_org_drug.standard == case_stnd]
                for row in df_org_drug_stnd.itertuples(name=None):
                    i, org, drug, stnd, sir, mic, mic_sign, mic_val, count = row
                    if sir in allowed_sirs:
                        entry = (org, drug, stnd)
                        if entry not in mic_ref_calls:
                            mic_ref_calls[entry] = {}
                        if mic not in mic_ref_calls[entry]:
                            mic_ref_calls[entry][mic] = {}
                        mic_ref_calls[entry][mic][sir] = count

    mic_ranges = {}                                      # {(org, drug, stnd): sir: [observed MICs]}
    for case in mic_ref_calls:
        mic_ranges[case] = {sir: [] for sir in allowed_sirs}
        for mic in mic_ref_calls[case]:
            for sir in mic_ref_calls[case][mic]:
                if '/' not in mic:
                    mic_ranges[case][sir].append(float(mic))
                else:
                    mic_ranges[case][sir].append(mic)
        for sir in allowed_sirs:
            if len(mic_ranges[case][sir]) == 0:
                del mic_ranges[case][sir]
            else:
                mic_ranges[case][sir] = sorted(mic_ranges[case][sir])
    return mic_ref_calls, mic_ranges


def validate_mic_sir_mappings(mic_ref_calls, mic_ranges):
    """Prints what is odd about the reference MIC calls of extract_mic_sir_mappings (reference :173-219): a MIC mapped to
    several SIRs of a case ('AMBIGUOUS MIC-SIR:'), a susceptible MIC that is not below every intermediate or resistant one
    or an intermediate one not below every resistant one ('INCONSISTENT S vs I:' ...), and the combination therapies. The
    text is what `print a, b` gave under Python 2 and print(a, b) gives under Python 3."""
    for case in sorted(mic_ref_calls.keys()):
        for mic in mic_ref_calls[case]:
            calls = mic_ref_calls[case][mic]
            if len(calls) > 1:
                print('AMBIGUOUS MIC-SIR:\t', '\t'.join(case), '\t', mic, mic_ref_calls[case][mic])

    for case in sorted(mic_ref_calls.keys()):
        is_combination_therapy = False
        for mic in mic_ref_calls[case]:
            for sir in mic_ref_calls[case][mic]:
                is_combination_therapy = is_combination_therapy or '/' in mic
        if not is_combination_therapy:
            has_s = 'susceptible' in mic_ranges[case]
            has_i = 'intermediate' in mic_ranges[case]
            has_r = 'resistant' in mic_ranges[case]
            if has_s and has_i:                          # check susceptible < intermediate
                s_vs_i = max(mic_ranges[case]['susceptible']) < min(mic_ranges[case]['intermediate'])
                if not s_vs_i:
                    print('INCONSISTENT S vs I:\t', '\t'.join(case), '\t', mic_ranges[case])
            if has_s and has_r:                          # check susceptible < resistant
                s_vs_r = max(mic_ranges[case]['susceptible']) < min(mic_ranges[case]['resistant'])
                if not s_vs_r:
                    print('INCONSISTENT S vs R:\t', '\t'.join(case), '\t', mic_ranges[case])
            if has_i and has_r:                          # check intermediate < resistant
                i_vs_r = max(mic_ranges[case]['intermediate']) < min(mic_ranges[case]['resistant'])
                if not i_vs_r:
                    print('INCONSISTENT I vs R:\t', '\t'.join(case), '\t', mic_ranges[case])
        else:
            print('COMBINATION THERAPY:\t', '\t'.join(case), '\t', mic_ranges[case])


# ---- interning: what the device path does with a column -------------------------------------------------------------------
def _codes(col, keep_nan_singleton=False):
    """int32 codes of a column (null = -1), equal exactly where Python's == on its values is true. Takes a numeric numpy
    column and an object column whose values are all strings; raises _Irregular for anything else (a column that mixes
    strings and numbers, other objects, extension dtypes). keep_nan_singleton: also insist that every null of an object
    column is the np.nan object, which is what makes the reference's tuples with a null equal."""
    values = col.values if isinstance(col, pd.Series) else col
    if not isinstance(values, np.ndarray):
        raise _Irregular('an extension array')
    if values.dtype == object:
        if pd.api.types.infer_dtype(values, skipna=True) not in ('string', 'empty'):
            raise _Irregular('a key column mixes strings and other values')
        if keep_nan_singleton:
            nulls = values[pd.isnull(values)]
            if nulls.size and set(map(id, nulls.tolist())) != {id(np.nan)}:
                raise _Irregular('a null that is not the np.nan object')
    elif values.dtype.kind not in 'iuf':
        raise _Irregular('a key column of dtype %s' % values.dtype)
    codes, uniques = pd.factorize(values)
    return codes.astype(np.int32), uniques


def _no_float_nan(col, codes, kept):
    values = col.values
    if values.dtype.kind == 'f' and (codes[kept] < 0).any():
        raise _Irregular('a float key column has a NaN in a kept row')


def _isin_codes(uniques, members):
    """bool per unique value: `value in members`, the test the reference's lambdas make"""
    return np.array([u in members for u in uniques.tolist()], dtype=bool)


def _org_of_rows(org_to_gids, df_amr, orgs):
    """int32 per row: the position in `orgs` of the organism that lists the row's genome, -1 for none"""
    org_of_gid = {}
    for o, org in enumerate(orgs):
        for gid in set(org_to_gids[org]):
            if pd.isnull(gid):
                raise _Irregular('a null genome id')
            if org_of_gid.setdefault(gid, o) != o:
                raise _Irregular('a genome is listed under two organisms')
    codes, uniques = _codes(df_amr.genome_id)
    of_unique = np.array([org_of_gid.get(u, -1) for u in uniques.tolist()] + [-1], dtype=np.int32)
    return of_unique[codes]                              # (code -1, a null, takes the appended -1)


def _group(ctx, columns, kept):
    """(rows, counts): the first row of every distinct tuple of `columns` among the rows `kept` (ascending, so in order of
    first appearance) and how many kept rows hold it"""
    if kept.size >= _TUPLE_MAX_ROWS:
        raise _Irregular('more rows than pgx_tuple_group takes')
    if kept.size == 0:
        return kept, np.zeros(0, dtype=np.int64)
    cols = np.ascontiguousarray(np.stack([c[kept] for c in columns]), dtype=np.int32)
    first, count, n_distinct = ctx.tuple_group(cols)
    reps = np.flatnonzero(first == np.arange(kept.size, dtype=first.dtype))
    if reps.size != n_distinct:
        raise RuntimeError('pgx_tuple_group: %d representatives, %d distinct' % (reps.size, n_distinct))
    return kept[reps], count[reps].astype(np.int64)


def _ordered_counts(values, counts):
    """what Series.value_counts gives for values with these counts in order of first appearance: pandas orders them"""
    return pd.Series(counts, index=pd.Index(values), dtype=np.int64).sort_values(ascending=False)


class _DrugCounts(object):
    """antibiotic.value_counts() of every organism's rows from one pgx_tuple_group over (organism, drug)"""

    def __init__(self, ctx, df_amr, org_row, n_orgs):
        self.drug_code, _ = _codes(df_amr.antibiotic)
        kept = np.flatnonzero((org_row >= 0) & (self.drug_code >= 0))
        _no_float_nan(df_amr.antibiotic, self.drug_code, org_row >= 0)
        rows, counts = _group(ctx, (org_row, self.drug_code), kept)
        drugs = df_amr.antibiotic.values
        self.per_org = []
        for o in range(n_orgs):
            sel = org_row[rows] == o
            series = _ordered_counts(drugs[rows[sel]], counts[sel])
            self.per_org.append((series, rows[sel], counts[sel]))

    def value_counts(self, o):
        return self.per_org[o][0]

    def target_mask(self, org_row, min_entries):
        """bool per row: its (organism, antibiotic) has at least min_entries rows"""
        n_drugs = int(self.drug_code.max()) + 1 if self.drug_code.size else 0
        ok = np.zeros((len(self.per_org), n_drugs + 1), dtype=bool)
        for o, (_, rows, counts) in enumerate(self.per_org):
            ok[o, self.drug_code[rows[counts >= min_entries]]] = True
        ok[:, n_drugs] = False
        return ok[np.maximum(org_row, 0), np.where(self.drug_code >= 0, self.drug_code, n_drugs)] & (org_row >= 0)


def extract_mic_calls(org_to_gids, df_amr, min_entries=100, ctx=None):
    """df_mic_calls: the distinct MIC measurements of every organism x drug case with at least min_entries rows, among the
    rows in mg/L from a laboratory method of ACCEPTED_MIC_METHODS whose standard is not in NULL_TESTING_STANDARDS (reference
    :222-284). Columns organism, drug, standard, sir, mic (as reported), mic_sign ('=' and '==' become np.nan), mic_val and
    count. org_to_gids: {organism: PATRIC genome ids}; df_amr: a frame in the layout of PATRIC_genomes_AMR.txt -- the
    columns genome_id, antibiotic, measurement, measurement_unit and laboratory_typing_method by name, and as in the
    reference the first eight columns and the fifth from the end (the standard) by position.
    The rows of an organism are sorted as Python 2 sorted them: a null standard, sir or mic_sign comes before every string
    (Python 3 raises TypeError where a null meets a string), everything else in Python's tuple order.
    ctx: a _native.Context for the device path. A genome listed under two organisms, a key column that mixes strings and
    numbers, a float key column with a NaN in a kept row, a null that is not the np.nan object and 2^24 rows or more go to
    the host loop."""
    rows = None
    if ctx is not None:
        try:
            rows = _mic_calls_device(ctx, org_to_gids, df_amr, min_entries)
        except _ENCODING_ERRORS:
            rows = None
    AMR_INFERENCE_PATH_COUNTS['mic_calls_host' if rows is None else 'mic_calls_device'] += 1
    if rows is None:
        rows = _mic_calls_host(org_to_gids, df_amr, min_entries)
    return pd.DataFrame(data=rows, columns=['organism', 'drug', 'standard', 'sir', 'mic', 'mic_sign', 'mic_val', 'count'])


def _py2_entry_key(entry):
    """the order Python 2 gave the counted tuples: None and NaN compared as smaller than every string"""
    org, drug, standard, sir, mic, mic_sign, mic_val = entry
    return (org, drug, (0, 0) if pd.isnull(standard) else (1, standard), (0, 0) if pd.isnull(sir) else (1, sir), mic,
            (0, 0) if pd.isnull(mic_sign) else (1, mic_sign), mic_val)


def _mic_call_entry(org, row):
    """the counted tuple of a row of itertuples(name=None), or None for a row that is not counted"""
    i, gid, gname, taxid, drug, sir, mic, mic_sign, mic_val = row[:9]
    if mic_sign in {'=', '=='}:
        mic_sign = np.nan
    standard = row[-5]
    if pd.notnull(mic):
        if standard not in NULL_TESTING_STANDARDS:
            return (org, drug, standard, sir, mic, mic_sign, mic_val)
    return None


def _mic_calls_host(org_to_gids, df_amr, min_entries):
    df_mic_calls = []
    for org in sorted(org_to_gids.keys()):
        gids = set(org_to_gids[org])
        df_org_amr = df_amr[df_amr.genome_id.map(lambda x: x in gids)]

        drug_counts = df_org_amr.antibiotic.value_counts()
        df = drug_counts[drug_counts >= min_entries]
        target_drugs = set(df.index)

        df_org_mic = df_org_amr[pd.notnull(df_org_amr.measurement)]
        df_org_mic = df_org_mic[df_org_mic.measurement_unit == 'mg/L']
        df_org_mic = df_org_mic[df_org_mic.antibiotic.map(lambda x: x in target_drugs)]
        df_org_mic = df_org_mic[df_org_mic.laboratory_typing_method.map(lambda x: x in ACCEPTED_MIC_METHODS)]

        mic_calls = []
        for row in df_org_mic.itertuples(name=None):
            entry = _mic_call_entry(org, row)
            if entry is not None:
                mic_calls.append(entry)
        mic_calls = collections.Counter(mic_calls)
        for entry in sorted(mic_calls.keys(), key=_py2_entry_key):
            df_mic_calls.append(list(entry) + [mic_calls[entry]])
    return df_mic_calls


def _mic_calls_device(ctx, org_to_gids, df_amr, min_entries):
    orgs = sorted(org_to_gids.keys())
    if df_amr.shape[1] < 8 or not df_amr.columns.is_unique:
        raise _Irregular('not the layout of a PATRIC AMR table')
    org_row = _org_of_rows(org_to_gids, df_amr, orgs)
    drug_counts = _DrugCounts(ctx, df_amr, org_row, len(orgs))

    # the row filters, as array operations on codes
    unit_code, units = _codes(df_amr.measurement_unit)
    method_code, methods = _codes(df_amr.laboratory_typing_method)
    is_mgl = np.append(np.array([u == 'mg/L' for u in units.tolist()], dtype=bool), False)
    is_method = np.append(_isin_codes(methods, ACCEPTED_MIC_METHODS), False)
    keep = drug_counts.target_mask(org_row, min_entries) & pd.notnull(df_amr.measurement.values)
    keep &= is_mgl[unit_code] & is_method[method_code]

    # the seven columns of a call, by position as in the reference
    positions = (3, -5, 4, 5, 6, 7)                      # drug, standard, sir, mic, mic_sign, mic_val
    series = [df_amr.iloc[:, p] for p in positions]
    coded = [_codes(s, keep_nan_singleton=True) for s in series]
    drug, standard, sir, mic, sign, val = (c for c, _ in coded)
    keep &= mic >= 0
    keep &= np.append(~_isin_codes(coded[1][1], NULL_TESTING_STANDARDS), True)[standard]
    # '=' and '==' are counted with the exact MICs, whose sign is null
    sign = np.where(np.append(_isin_codes(coded[4][1], {'=', '=='}), False)[sign], -1, sign).astype(np.int32)
    for s, c in zip(series, (drug, standard, sir, mic, coded[4][0], val)):
        _no_float_nan(s, c, keep)
    _no_float_nan(df_amr.measurement_unit, unit_code, org_row >= 0)
    _no_float_nan(df_amr.laboratory_typing_method, method_code, org_row >= 0)
    rows, counts = _group(ctx, (org_row, drug, standard, sir, mic, sign, val), np.flatnonzero(keep))

    # only the distinct calls are decoded (by the reference's own statements, on their first rows) and ordered
    per_org = [[] for _ in orgs]
    for row, o, count in zip(df_amr.iloc[rows].itertuples(name=None), org_row[rows].tolist(), counts.tolist()):
        per_org[o].append((_mic_call_entry(orgs[o], row), count))
    df_mic_calls = []
    for calls in per_org:
        for entry, count in sorted(calls, key=lambda c: _py2_entry_key(c[0])):
            df_mic_calls.append(list(entry) + [count])
    return df_mic_calls


def extract_primary_stnds(org_to_gids, df_amr, min_entries=100, stnd_col='testing_standard', ctx=None):
    """df_primary_stnds: the most common testing standard of every organism x drug case with at least min_entries rows
    (reference :287-347), indexed by 'organism|antibiotic'. Columns top_stnd (the most common non-null standard; null only
    when there is no other), n_top_stnd, n_other_stnd (rows under other non-null standards), n_missing_stnd (rows without
    one) and other_stnds (the other non-null standards joined by ';' in the order of their counts, np.nan for none).
    The reference takes len() of a filter(), which Python 3 refuses with TypeError; this has the Python 2 meaning. The top
    standard, the order of other_stnds and every tie are what pandas' value_counts(dropna=False) gives.
    ctx: a _native.Context for the device path, which hands pandas the device's counts in order of first appearance and lets
    it order them. Irregular input (see extract_mic_calls) goes to the host loop."""
    orgs = sorted(org_to_gids.keys())
    plan = None
    if ctx is not None:
        try:
            plan = _StandardCounts(ctx, org_to_gids, df_amr, orgs, stnd_col)
        except _ENCODING_ERRORS:
            plan = None
    AMR_INFERENCE_PATH_COUNTS['primary_stnds_host' if plan is None else 'primary_stnds_device'] += 1

    df_primary_stnds = {}
    for o, org in enumerate(orgs):
        if plan is None:
            org_gids = set(org_to_gids[org])
            df_org_amr = df_amr[df_amr.genome_id.map(lambda x: x in org_gids)]
            drug_counts = df_org_amr.antibiotic.value_counts()
        else:
            drug_counts = plan.drug_counts.value_counts(o)
        df = drug_counts[drug_counts >= min_entries]
        target_drugs = set(df.index)

        for drug in target_drugs:
            if plan is None:
                df_drug_amr = df_org_amr[df_org_amr.antibiotic == drug]
                stnd_counts = df_drug_amr[stnd_col].value_counts(dropna=False)
                n_rows = df_drug_amr.shape[0]
            else:
                stnd_counts = plan.value_counts(o, drug)
                n_rows = int(drug_counts[drug])
            top_stnd = stnd_counts.index[0]
            top_stnd = stnd_counts.index[1] if pd.isnull(top_stnd) and stnd_counts.shape[0] > 1 else top_stnd
            other_stnds = list(filter(lambda x: pd.notnull(x) and x != top_stnd, stnd_counts.index.tolist()))
            n_top_stnd = stnd_counts[top_stnd]
            n_missing = stnd_counts.loc[np.nan] if np.nan in stnd_counts.index else 0
            n_other_stnd = n_rows - n_top_stnd * (pd.notnull(top_stnd)) - n_missing
            other_stnds_out = ';'.join(other_stnds) if len(other_stnds) > 0 else np.nan
            df_primary_stnds[org + '|' + drug] = {
                'top_stnd': top_stnd,
                'n_top_stnd': n_top_stnd,
                'n_other_stnd': n_other_stnd,
                'n_missing_stnd': n_missing,
                'other_stnds': other_stnds_out
            }
    df_primary_stnds = pd.DataFrame.from_dict(df_primary_stnds, orient='index')
    df_primary_stnds = df_primary_stnds.reindex(columns=['top_stnd', 'n_top_stnd', 'n_other_stnd', 'n_missing_stnd',
                                                         'other_stnds'])
    return df_primary_stnds


class _StandardCounts(object):
    """stnd_col.value_counts(dropna=False) of every organism x drug case from one pgx_tuple_group over (organism, drug,
    standard), beside the drug counts"""

    def __init__(self, ctx, org_to_gids, df_amr, orgs, stnd_col):
        org_row = _org_of_rows(org_to_gids, df_amr, orgs)
        self.drug_counts = _DrugCounts(ctx, df_amr, org_row, len(orgs))
        stnd = df_amr[stnd_col]
        if not isinstance(stnd, pd.Series):
            raise _Irregular('stnd_col names several columns')
        stnd_code, _ = _codes(stnd, keep_nan_singleton=True)
        drug_code = self.drug_counts.drug_code
        kept = (org_row >= 0) & (drug_code >= 0)
        _no_float_nan(stnd, stnd_code, kept)
        rows, counts = _group(ctx, (org_row, drug_code, stnd_code), np.flatnonzero(kept))
        drugs, self.stnds = df_amr.antibiotic.values, stnd.values
        self.cases = {}
        for row, count in zip(rows.tolist(), counts.tolist()):
            self.cases.setdefault((int(org_row[row]), drugs[row]), []).append((row, count))

    def value_counts(self, o, drug):
        rows, counts = zip(*self.cases[(o, drug)])
        return _ordered_counts(self.stnds[list(rows)], list(counts))


# ---- inference over a table -------------------------------------------------------------------------------------------------
def infer_sir_batch(orgs, antibiotics, measurement_values, measurement_signs, mic_ranges, df_case_to_standard, ctx=None):
    """(sir, primary_stnd), two object arrays: element i is exactly what infer_sir(orgs[i], antibiotics[i],
    measurement_values[i], measurement_signs[i], mic_ranges, df_case_to_standard) returns. Not in the reference, whose
    scalar function is called once per row. The four arguments are taken as np.asarray(x, dtype=object), so the identity of
    their elements (the np.nan object among the signs) carries over. If infer_sir would raise for some row, the call raises
    what the first such row raises.
    ctx: a _native.Context for the device path: cases, classes and observed MICs flattened, the rows encoded, one
    pgx_mic_infer. A duplicate index of df_case_to_standard, an organism or drug that is no string, a measurement value that
    is neither str nor float, a list element that is neither, a row the kernel cannot decide (a range test on a class with a
    string MIC, where the reference raises) and sizes past the kernel's limits go to the host loop."""
    columns = [np.asarray(x, dtype=object) for x in (orgs, antibiotics, measurement_values, measurement_signs)]
    if any(c.ndim != 1 or c.shape != columns[0].shape for c in columns):
        raise ValueError('orgs, antibiotics, measurement_values and measurement_signs must be 1-D and of one length')
    out = None
    if ctx is not None:
        try:
            out = _infer_device(ctx, columns, mic_ranges, df_case_to_standard)
        except _ENCODING_ERRORS:
            out = None
    AMR_INFERENCE_PATH_COUNTS['infer_sir_batch_host' if out is None else 'infer_sir_batch_device'] += 1
    if out is None:
        n = columns[0].size
        out = np.empty(n, dtype=object), np.empty(n, dtype=object)
        for i, (org, antibiotic, value, sign) in enumerate(zip(*columns)):
            out[0][i], out[1][i] = infer_sir(org, antibiotic, value, sign, mic_ranges, df_case_to_standard)
    return out


_SIGN_CODES = {np.nan: 0, '=': 0, '==': 0, '<': 1, '<=': 1, '>': 2, '>=': 2}   # looked up as the reference's sets are


def _all_str(values):
    return all(type(v) is str for v in values)


def _infer_device(ctx, columns, mic_ranges, df_case_to_standard):
    orgs, antibiotics, values, signs = columns
    n = orgs.size
    if n >= _MIC_MAX_ROWS:
        raise _Irregular('more rows than pgx_mic_infer takes')
    if not isinstance(df_case_to_standard, pd.Series) or not isinstance(mic_ranges, dict):
        raise _Irregular('df_case_to_standard is no Series or mic_ranges no dict')
    if not df_case_to_standard.index.is_unique:
        raise _Irregular('df_case_to_standard has a duplicate index')
    try:
        org_code, org_names = pd.factorize(orgs)
        ab_code, ab_names = pd.factorize(antibiotics)
        sign_code = np.frompyfunc(_SIGN_CODES.get, 2, 1)(signs, 3).astype(np.uint8) if n else np.zeros(0, dtype=np.uint8)
    except TypeError:
        raise _Irregular('an unhashable organism, drug or sign')
    org_names, ab_names = org_names.tolist(), ab_names.tolist()
    if (org_code < 0).any() or (ab_code < 0).any() or not _all_str(org_names) or not _all_str(ab_names):
        raise _Irregular('an organism or drug that is no string')

    # the cases: one per distinct (organism, drug) pair that has a standard and ranges
    pair = org_code.astype(np.int64) * max(len(ab_names), 1) + ab_code
    pairs, pair_row = np.unique(pair, return_inverse=True)
    class_begin, sir_code, role, fl_begin, tk_begin, fvals, tvals = [0], [], [], [0], [0], [], []
    sir_names, sir_id, token_id, case_stnd, case_of_pair = [], {}, {}, [], np.full(pairs.size, -1, dtype=np.int32)
    for p, key in enumerate(pairs.tolist()):
        org, antibiotic = org_names[key // max(len(ab_names), 1)], ab_names[key % max(len(ab_names), 1)]
        case = org + '|' + antibiotic
        try:
            if case not in df_case_to_standard.index:
                continue
            primary_stnd = df_case_to_standard[case]
            entry = (org, antibiotic, primary_stnd)
            if entry not in mic_ranges:
                continue
        except TypeError:
            raise _Irregular('a standard that cannot be looked up')
        case_of_pair[p] = len(case_stnd)
        case_stnd.append(primary_stnd)
        if not isinstance(mic_ranges[entry], dict):
            raise _Irregular('the classes of a case are no dict')
        for sir in mic_ranges[entry]:
            mics = mic_ranges[entry][sir]
            if not isinstance(mics, (list, tuple)) or not isinstance(sir, str):
                raise _Irregular('a class that is no string or whose MICs are no list')
            floats = sorted(float(m) for m in mics if isinstance(m, float))
            strings = [m for m in mics if type(m) is str]
            if len(floats) + len(strings) != len(mics) or any(f != f for f in floats):
                raise _Irregular('an observed MIC that is neither str nor float, or a NaN')
            if sir not in sir_id:
                sir_id[sir] = len(sir_names)
                sir_names.append(sir)
            sir_code.append(sir_id[sir])
            role.append(0 if sir == 'susceptible' else 1 if sir == 'resistant' else 2)
            fvals.extend(floats)
            tvals.extend(sorted(token_id.setdefault(s, len(token_id)) for s in strings))
            fl_begin.append(len(fvals))
            tk_begin.append(len(tvals))
        class_begin.append(len(sir_code))
    if max(len(case_stnd), len(sir_code), len(fvals), len(tvals)) >= _MIC_MAX_TABLE:
        raise _Irregular('more cases, classes or observed MICs than pgx_mic_infer takes')

    # the rows: measurement values are strings (a key among the string MICs, a number where float() takes them) or floats
    is_str = np.frompyfunc(lambda v: type(v) is str, 1, 1)(values).astype(bool) if n else np.zeros(0, dtype=bool)
    is_float = np.frompyfunc(lambda v: isinstance(v, float), 1, 1)(values).astype(bool) if n else np.zeros(0, dtype=bool)
    if not (is_str | is_float).all():
        raise _Irregular('a measurement value that is neither str nor float')
    kind = is_float.astype(np.uint8)
    value = np.zeros(n, dtype=np.float64)
    token = np.full(n, -1, dtype=np.int32)
    numeric = np.ones(n, dtype=bool)
    value[is_float] = values[is_float].astype(np.float64)
    if is_str.any():
        str_code, strings = pd.factorize(values[is_str])
        s_value, s_numeric, s_token = np.zeros(len(strings)), np.ones(len(strings), dtype=bool), np.full(len(strings), -1, np.int32)
        for j, s in enumerate(strings.tolist()):
            try:
                s_value[j] = float(s)
            except ValueError:
                s_numeric[j] = False
            s_token[j] = token_id.get(s, -1)
        value[is_str], numeric[is_str], token[is_str] = s_value[str_code], s_numeric[str_code], s_token[str_code]
    ab_combo = np.array([__is_combination_therapy__(a) for a in ab_names], dtype=bool)
    combo = (ab_combo[ab_code] | ~numeric).astype(np.uint8) if n else np.zeros(0, dtype=np.uint8)
    case = case_of_pair[pair_row].astype(np.int32) if n else np.zeros(0, dtype=np.int32)

    codes = ctx.mic_infer(np.array(class_begin, dtype=np.uint32), np.array(sir_code, dtype=np.int32),
                          np.array(role, dtype=np.uint8), np.array(fl_begin, dtype=np.uint32), np.array(tk_begin, dtype=np.uint32),
                          np.array(fvals, dtype=np.float64), np.array(tvals, dtype=np.int32), case, sign_code, combo, kind, token,
                          value)
    if (codes == -2).any():
        raise _Irregular('a row the kernel leaves to the host')
    sir_of = np.empty(len(sir_names) + 1, dtype=object)
    sir_of[:-1], sir_of[-1] = sir_names, np.nan
    stnd_of = np.empty(len(case_stnd) + 1, dtype=object)
    for c, s in enumerate(case_stnd):
        stnd_of[c] = s
    stnd_of[-1] = np.nan
    hit = codes >= 0
    return sir_of[np.where(hit, codes, -1)], stnd_of[np.where(hit, case, -1)]


def __is_combination_therapy__(antibiotic):
    """Check if an antibiotic is a combination therapy"""
    if antibiotic == 'polymyxin_b' or antibiotic == 'nalidixic_acid':
        return False
    elif '_' in antibiotic:
        return True
    else:
        return False
