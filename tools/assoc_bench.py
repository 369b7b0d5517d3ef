#!/usr/bin/env python
"""Timing of the association screen on the device. Prints one JSON object.

    python tools/assoc_bench.py [--runs 5] [--drugs 32] [--out profiles/assoc_bench.json]

On synth.pancore_matrix(150000, 400, 1), median / min / max of --runs runs after a warm-up, and beside each figure the
same work by tests/assoc_model.py (numpy, one thread) on this host:
  compress_rows_spmatrix     the public call on the COO matrix (upload, device blocks, CSR of the representatives, lists)
  contingency_1 / _32        contingency_tables_from_sparse with 1 and with 32 target vectors (one pass each)
  screen_32_drugs            prepare_amr_case_data + prefilter_features_by_lor for every one of --drugs seeded random
                             phenotype columns (30 % NaN each), the table resident on the device (uploaded once, before
                             the clock starts, as a pipeline leaves it); model: assoc_model.screen per drug on the dense
                             bool table
  device_passes              what the device part alone takes, from the resident bitmap: blocks, 32-target contingency,
                             one drug's selected + drop-empty blocks (host clock around the library call, which ends
                             in a stream synchronise)
  kernel_ms                  per-kernel time of ONE profiled run of those three passes (pgx_profile_read; a run of its own)
  algorithmic_gb             signature image bytes a step reads once (rows x words x 8), and the rate that makes of the
                             32-target contingency kernel's time (32 reads of the image) -- against the 8.0 TB/s of HBM
                             as a yardstick only: the image is cache-resident
The condition of DESIGN 6d: every device figure below its model figure of this run ("device_faster").
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from pangenomix_amd import _native, ml_pipelines, sparse_utils, synth           # noqa: E402

HBM_TB_PER_S = 8.0


def timed(fn, runs, warm=True):
    if warm:
        fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return {'median': float(np.median(t)), 'min': min(t), 'max': max(t)}, out


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--drugs', type=int, default=32)
    ap.add_argument('--rows', type=int, default=150000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import assoc_model
    ctx = _native.Context(0)
    rng = np.random.default_rng(7)
    S = 400
    r, c, G = synth.pancore_matrix(args.rows, S, 1)
    coo = scipy.sparse.coo_matrix((np.ones(r.size, dtype=np.int64), (r, c)), shape=(G, S))
    X = assoc_model.dense(r, c, (G, S))
    out = {'device': ctx.device_info()['name'], 'runs': args.runs, 'shape': [G, S], 'ones': int(r.size)}

    # (a) blocks
    dev, (spblock, defs) = timed(lambda: sparse_utils.compress_rows_spmatrix(coo, ctx=ctx), args.runs)
    mod, (b_model, rep_model) = timed(lambda: assoc_model.blocks(X), args.runs)
    assert spblock.shape[0] == rep_model.size and [int(x[0]) for x in defs] == rep_model.tolist()
    out['compress_rows_spmatrix'] = {'device_s': dev, 'model_s': mod, 'blocks': int(rep_model.size),
                                     'device_faster': dev['median'] < mod['median']}

    # (b) contingency, 1 and 32 targets
    targets = (rng.random((32, S)) < 0.4).astype(float)
    for name, tg in (('contingency_1', targets[0]), ('contingency_32', targets)):
        dev, got = timed(lambda: ml_pipelines.contingency_tables_from_sparse(coo, tg, ctx=ctx), args.runs)
        model_fn = (lambda: assoc_model.contingency(X, tg)) if tg.ndim == 1 else \
            (lambda: np.stack([assoc_model.contingency(X, t) for t in tg]))
        mod, want = timed(model_fn, args.runs)
        assert np.array_equal(got, want)
        out[name] = {'device_s': dev, 'model_s': mod, 'device_faster': dev['median'] < mod['median']}

    # (c) the whole screen for --drugs drugs from the resident table
    token = ctx.bitmap_from_clusters(r, np.arange(r.size), c.astype(np.uint32), np.arange(S), G, S)
    lsdf = sparse_utils.LightSparseDataFrame(np.array(['g%d' % i for i in range(G)]), np.array(['s%d' % j for j in range(S)]), coo)
    lsdf._pgx_resident = {'ctx': ctx, 'token': token, 'shape': lsdf.shape, 'data': lsdf.data, 'nnz': int(lsdf.data.nnz),
                          'row_cluster': np.arange(G, dtype=np.int32)}
    pheno = (rng.random((S, args.drugs)) < 0.4).astype(float)
    pheno[rng.random((S, args.drugs)) < 0.3] = np.nan
    drugs = ['drug%d' % k for k in range(args.drugs)]
    df_amr = pd.DataFrame(pheno, index=lsdf.columns, columns=drugs)
    df_known = pd.DataFrame(np.ones((2, args.drugs)), index=lsdf.index[:2], columns=drugs)

    def device_screen():
        kept = []
        for drug in drugs:
            amr, _, _, block, _ = quiet(ml_pipelines.prepare_amr_case_data, drug, lsdf, df_amr, df_known, ctx=ctx)
            kept.append(list(quiet(ml_pipelines.prefilter_features_by_lor, block, amr, ctx=ctx).index))
        return kept

    def model_screen():
        return [['B%d' % i for i in assoc_model.screen(X, pheno[:, k])[4]] for k in range(args.drugs)]

    runs_c = max(1, min(args.runs, 3))
    dev, kept_dev = timed(device_screen, runs_c)
    mod, kept_mod = timed(model_screen, runs_c, warm=False)
    assert kept_dev == kept_mod
    out['screen_%d_drugs' % args.drugs] = {'device_s': dev, 'model_s': mod, 'runs': runs_c,
                                           'features_kept': [len(k) for k in kept_dev],
                                           'device_faster': dev['median'] < mod['median']}

    # the device part alone, from the resident bitmap
    row_map = lsdf._pgx_resident['row_cluster']
    masks32 = ml_pipelines._target_masks(targets)
    cols0 = np.flatnonzero(pheno[:, 0] == pheno[:, 0])
    passes = {'blocks': lambda: ctx.assoc_resident(token, row_map, S, blocks=True),
              'contingency_32': lambda: ctx.assoc_resident(token, row_map, S, masks=masks32),
              'drug_blocks': lambda: ctx.assoc_resident(token, row_map, S, col_map=cols0, blocks=True, drop_empty=True)}
    out['device_passes'] = {k: timed(fn, args.runs)[0] for k, fn in passes.items()}
    ctx.profile(True)
    ctx.profile_reset()
    for fn in passes.values():
        fn()
    kern = {k: {'ms': ms, 'launches': n} for k, (ms, n) in ctx.profile_read().items() if k.startswith('assoc_')}
    ctx.profile(False)
    out['kernel_ms'] = kern
    image = G * ((S + 63) // 64) * 8
    out['algorithmic_gb'] = {'signature_image': image / 1e9}
    if kern.get('assoc_tp_kernel', {}).get('ms', 0) > 0:          # 32 targets: the image is read 32 times by one launch
        rate = 32 * image / (kern['assoc_tp_kernel']['ms'] * 1e-3) / 1e12
        out['algorithmic_gb']['assoc_tp_kernel_tb_per_s_cache_resident'] = rate
        out['algorithmic_gb']['assoc_tp_kernel_share_of_hbm_8_tb_per_s'] = rate / HBM_TB_PER_S
    ctx.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
