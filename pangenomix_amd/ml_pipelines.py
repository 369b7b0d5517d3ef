"""
The per-phenotype association screen on MI355X.

Mirror of the part of the reference's ml_pipelines.py that consumes the feature x genome table before any model is
trained: `prepare_amr_case_data` (pick the genomes that have a phenotype for a drug, drop the features that are now
empty, merge features with identical occurrence into blocks), `contingency_tables_from_sparse` (TP / FP / FN / TN of
every feature against a phenotype vector), `adjusted_lor` and `prefilter_features_by_lor`. Same names, positional order
and defaults; `ctx` is the only addition.

All of it is integer work on the genome-major bitmap libpgx builds and keeps resident (pangenomix_amd/csrc/assoc.hip,
DESIGN.md 6d): the rows' bits among the selected genomes, AND + popcount against the phenotype masks, equality of rows.
The device returns integers; the float columns of the contingency table and the one log2 are formed on the host with
the reference's expressions. The reference densifies the table in batches. There is no CPU fallback. The model half
of the reference's module (evaluate_model and its helpers) is not part of this package; nothing here imports sklearn.
"""

from __future__ import print_function

import numpy as np

from . import sparse_utils


def _target_masks(targets):
    """uint64 [n_targets, ceil(n_samples / 64) or 1]: bit j of row t = targets[t, j] is non-zero (np.logical_and's
    reading of a number: a NaN counts)."""
    n_targets, n_samples = targets.shape
    words = max(1, (n_samples + 63) // 64)
    bits = np.zeros((n_targets, words * 64), dtype=bool)
    bits[:, :n_samples] = targets != 0
    return np.packbits(bits, axis=1, bitorder='little').view('<u8').astype(np.uint64, copy=False)


def contingency_tables_from_sparse(sp_features, target, batch_size=10000, ctx=None):
    """Contingency tables between every feature (row) of a binary feature x sample table and a target vector.

    sp_features : scipy.sparse matrix, dense 2-D array of 0/1 or LightSparseDataFrame (never densified)
    target      : one value per sample; a sample counts as positive where the value is non-zero (a NaN too). A 2-D
                  array (n_targets, n_samples) screens all its rows in ONE pass over the table.
    batch_size  : accepted for compatibility and ignored
    ctx         : optional pangenomix_amd._native.Context (default: process-wide)

    Returns float64 (n_features, 4): TP, FP, FN, TN per feature -- TP and the features' incidence are counted on the device,
    FP = incidence - TP, FN = target.sum() - TP, TN = n_samples - TP - FP - FN as the reference forms them -- or
    (n_targets, n_features, 4), whose row t equals the call with target[t].
    """
    who = 'contingency_tables_from_sparse'
    table = sparse_utils._screen_table(sp_features, who)
    n_features, n_samples = table[2]
    target = np.asarray(target)
    targets = target[None, :] if target.ndim == 1 else target
    if targets.ndim != 2 or targets.shape[1] != n_samples:
        raise ValueError('target must hold one value per sample')
    out = sparse_utils._screen(table, who, ctx, masks=_target_masks(targets))
    incidence = out['incidence'].astype(np.int64)
    contingency = np.zeros((targets.shape[0], n_features, 4))
    for t in range(targets.shape[0]):
        positives = float(targets[t].sum())
        TPs = out['tp'][t].astype(np.int64)
        FPs = incidence - TPs
        FNs = positives - TPs
        TNs = n_samples - TPs - FPs - FNs
        contingency[t, :, 0] = TPs
        contingency[t, :, 1] = FPs
        contingency[t, :, 2] = FNs
        contingency[t, :, 3] = TNs
    return contingency[0] if target.ndim == 1 else contingency


def adjusted_lor(contingency):
    """Adjusted log2 odds ratio of every row of a contingency table (TP, FP, FN, TN), as defined in
    https://doi.org/10.1371/journal.pcbi.1007608: each cell is offset by the positive / negative rate."""
    TPs, FPs = contingency[:, 0], contingency[:, 1]
    FNs, TNs = contingency[:, 2], contingency[:, 3]
    PRs = np.divide(TPs + FNs, contingency.sum(axis=1, dtype='float'))
    NRs = 1.0 - PRs
    numerator = np.multiply(TPs + PRs, TNs + NRs)
    denominator = np.multiply(FPs + NRs, FNs + PRs)
    return np.log2(np.divide(numerator, denominator))


def _select_by_lor(lors, max_features):
    """Row positions kept by the LOR filter: half = max_features // 2; the rows ordered by LOR descending with a STABLE
    sort (equal LORs keep ascending position, NaN last); the first `half` of that order, then its last `half`."""
    order = np.argsort(-np.asarray(lors, dtype=np.float64), kind='stable')
    half = int(max_features) // 2
    return order[:half].tolist() + order[order.size - half:].tolist()


def prefilter_features_by_lor(lsdf_case_block, df_amr_org_drug, min_freq=3, max_features=10000, ctx=None):
    """Filter compressed features by raw frequency and LOR: with 10000 features allowed, the 5000 with the highest and the
    5000 with the lowest LOR are kept.

    lsdf_case_block : LightSparseDataFrame, block x genome table from prepare_amr_case_data()
    df_amr_org_drug : pd.Series, phenotypes by genome from prepare_amr_case_data()
    min_freq        : minimum occurrence of a feature (default 3; 0 = no frequency filter)
    max_features    : maximum number of features returned (default 10000)

    The selection among more than max_features rows is this package's own rule (_select_by_lor): the
    reference's line raises TypeError under Python 3, and its unstable sort leaves the order of equal LORs open.
    """
    if min_freq > 0:
        feature_freqs = np.array(lsdf_case_block.data.sum(axis=1))[:, 0]
        count_filtered = np.where(feature_freqs >= min_freq)[0]
        lsdf = lsdf_case_block.islice(i_indices=count_filtered)
    else:
        lsdf = lsdf_case_block
    if lsdf.shape[0] <= max_features:
        return lsdf
    contingency = contingency_tables_from_sparse(lsdf.data, df_amr_org_drug.values.astype(float), batch_size=10000, ctx=ctx)
    lors = adjusted_lor(contingency)
    lsdf_case_block2 = lsdf.islice(i_indices=_select_by_lor(lors, max_features))
    print('Species x drug LOR-selected compressed features:', lsdf_case_block2.shape)
    return lsdf_case_block2


def prepare_amr_case_data(drug, lsdf_features, df_amr_org, df_known_amr, ctx=None):
    """The data of one species x drug case: the drug's phenotypes (genomes without one dropped), the known AMR features
    of the drug, the feature table reduced to those genomes and to the features that occur in them, and that table with
    features of identical occurrence merged into blocks.

    drug          : name of the antimicrobial (a column of df_amr_org and df_known_amr)
    lsdf_features : LightSparseDataFrame, feature x genome table
    df_amr_org    : pd.DataFrame, genome x drug phenotypes (NaN = none)
    df_known_amr  : pd.DataFrame, feature x drug table of known AMR features

    Returns (df_amr_org_drug, known_amr_drug_set, lsdf_case_features, lsdf_case_block, case_block_defs);
    case_block_defs[i] = the labels of the features in block i. For the gene table returned by build_cds_pangenome()
    the column selection, the empty-row drop and the blocks come from ONE pass over the bitmap the pipeline left on
    the device (nothing of the table is uploaded).
    """
    who = 'prepare_amr_case_data'
    df_amr_org_drug = df_amr_org.loc[:, drug].dropna()
    print('Species x drug AMR data:', df_amr_org_drug.shape)
    df_known_amr_drug = df_known_amr.loc[:, drug].dropna()
    known_amr_drug_set = set(df_known_amr_drug.index)
    print('Species x drug AMR features:', len(known_amr_drug_set))

    table = sparse_utils._screen_table(lsdf_features, who)
    if table[3] is not None and table[2][0] > 0 and len(df_amr_org_drug) > 0:
        i_columns = [lsdf_features.column_map[x] for x in df_amr_org_drug.keys()]
        out = sparse_utils._screen(table, who, ctx, col_map=i_columns, blocks=True, drop_empty=True)
        kept = np.where(out['incidence'] > 0)[0]
        # labelslice + drop_empty in one: columns by CSC, kept rows by CSR (the matrices the two calls would build)
        case = lsdf_features.data.tocsc()[:, i_columns].tocsr()[kept, :]
        lsdf_case_features = sparse_utils.LightSparseDataFrame(lsdf_features.index[kept], lsdf_features.columns[i_columns], case)
        print('Species x drug reduced features:', lsdf_case_features.shape)
        position = np.cumsum(out['incidence'] > 0) - 1        # a kept row's position in the reduced table
        lsdf_case_block, case_block_defs = sparse_utils._block_frame(lsdf_case_features, out['block_of_row'][kept],
                                                                     position[out['rep_row']], case)
    else:
        lsdf_case_features = lsdf_features.labelslice(columns=df_amr_org_drug.keys())
        lsdf_case_features = lsdf_case_features.drop_empty(axis='index')
        print('Species x drug reduced features:', lsdf_case_features.shape)
        lsdf_case_block, case_block_defs = sparse_utils.compress_rows(lsdf_case_features, ctx=ctx)
    print('Species x drug compressed features:', lsdf_case_block.shape)
    return df_amr_org_drug, known_amr_drug_set, lsdf_case_features, lsdf_case_block, case_block_defs
