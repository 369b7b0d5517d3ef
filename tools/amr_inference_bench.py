#!/usr/bin/env python
"""Timing of amr_inference.extract_primary_stnds, extract_mic_calls and infer_sir_batch with and without a device context
(DESIGN.md section 6o). Prints one JSON object.

    python tools/amr_inference_bench.py [--rows 1000000] [--runs 3] [--out profiles/amr_inference_bench.json]

The input is synthetic (pangenomix_amd.synth.patric_amr_table): --rows rows in PATRIC's layout over --orgs organisms of
--genomes genomes each and --drugs drugs. The real PATRIC_genomes_AMR.txt is of the order of 10^6 rows; its size was not
measured, and the record states the size that was used.
Every device result is first compared with the host's (frames under assert_frame_equal, arrays element by element) and
AMR_INFERENCE_PATH_COUNTS must name the device path. Then, in one process on one machine, after one warm-up call each:
  primary_stnds_device / _host   extract_primary_stnds(ctx=ctx) / (ctx=None): median / min / max of --runs / --host-runs calls
  mic_calls_device / _host       extract_mic_calls likewise
  infer_batch_device / _host     infer_sir_batch likewise, on every row of an organism that has a measurement
  *_stages                       where the time of ONE device call goes: interning and filters on the host, the library calls,
                                 the decoding and ordering on the host (host clocks around each; the library calls synchronise)
  tuple_group, mic_infer         the library calls alone on this input's arrays (upload, kernels, download)
  kernel_ms                      per-kernel time of ONE profiled run of the three device calls (pgx_profile_read), a run of its own
The host paths are THIS PROJECT'S restatement of the reference's loops (ctx=None). The reference itself does not run under
Python 3; no figure is given for it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pangenomix_amd import _native, synth                          # noqa: E402
from pangenomix_amd import amr_inference as ai                     # noqa: E402


def timed(fn, runs):
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return {'median': float(np.median(t)), 'min': min(t), 'max': max(t), 'runs': runs}, out


def note(what):
    print('[amr_inference_bench] ' + what, file=sys.stderr, flush=True)


class Clocked(object):
    """a context whose two library calls are timed and whose arguments are kept: what the device path spends in the library"""

    def __init__(self, ctx):
        self.ctx, self.seconds, self.args = ctx, {'tuple_group': 0.0, 'mic_infer': 0.0}, {}

    def tuple_group(self, cols, flags=0):
        t0 = time.perf_counter()
        out = self.ctx.tuple_group(cols, flags)
        self.seconds['tuple_group'] += time.perf_counter() - t0
        self.args.setdefault('tuple_group', []).append(cols)
        return out

    def mic_infer(self, *arrays):
        t0 = time.perf_counter()
        out = self.ctx.mic_infer(*arrays)
        self.seconds['mic_infer'] += time.perf_counter() - t0
        self.args['mic_infer'] = arrays
        return out


def same_arrays(a, b):
    return all(len(x) == len(y) and all(p is q or p == q for p, q in zip(x.tolist(), y.tolist())) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1000000)
    ap.add_argument('--orgs', type=int, default=8)
    ap.add_argument('--genomes', type=int, default=2000)
    ap.add_argument('--drugs', type=int, default=40)
    ap.add_argument('--min-entries', type=int, default=100)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--host-runs', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = _native.Context(0)
    org_to_gids, df = synth.patric_amr_table(args.rows, args.orgs, args.genomes, args.drugs)
    out = {'device': ctx.device_info()['name'], 'rows': args.rows, 'organisms': args.orgs, 'genomes_per_organism': args.genomes,
           'drugs': args.drugs, 'min_entries': args.min_entries,
           'size_note': 'synthetic table of `rows` rows; the real PATRIC_genomes_AMR.txt is of the order of 10^6 rows (not measured)',
           'host_path_is': "this project's restatement of the reference's loops (ctx=None)"}
    note('table of %d rows made' % len(df))

    def compare(name, fn, same):
        ai.AMR_INFERENCE_PATH_COUNTS.clear()
        clocked = Clocked(ctx)
        t0 = time.perf_counter()
        got = fn(clocked)
        first = time.perf_counter() - t0
        assert dict(ai.AMR_INFERENCE_PATH_COUNTS) == {name + '_device': 1}, dict(ai.AMR_INFERENCE_PATH_COUNTS)
        out[name + '_host'], want = timed(lambda: fn(None), args.host_runs)
        same(got, want)
        out[name + '_device'], _ = timed(lambda: fn(ctx), args.runs)
        out[name + '_first_device_call'] = first
        clocked = Clocked(ctx)
        t0 = time.perf_counter()
        fn(clocked)
        total = time.perf_counter() - t0
        library = sum(clocked.seconds.values())
        out[name + '_stages'] = {'whole_call': total, 'library_calls': library, 'host_encode_decode': total - library}
        out[name + '_speedup_host_median_over_device_median'] = out[name + '_host']['median'] / out[name + '_device']['median']
        note('%s: device %.3f s (library %.3f s), host %.3f s' % (name, out[name + '_device']['median'], library,
                                                                out[name + '_host']['median']))
        return want, clocked

    stnds, c1 = compare('primary_stnds', lambda c: ai.extract_primary_stnds(org_to_gids, df, args.min_entries, ctx=c),
                        pd.testing.assert_frame_equal)
    calls, c2 = compare('mic_calls', lambda c: ai.extract_mic_calls(org_to_gids, df, args.min_entries, ctx=c),
                        pd.testing.assert_frame_equal)
    out['cases'], out['distinct_mic_calls'] = int(len(stnds)), int(len(calls))
    case_to_standard = stnds.top_stnd
    _, mic_ranges = ai.extract_mic_sir_mappings(calls, case_to_standard)
    org_of = {gid: org for org, gids in org_to_gids.items() for gid in gids}
    asked = df[df.genome_id.isin(list(org_of)).values & pd.notnull(df.measurement_value).values]
    columns = (asked.genome_id.map(org_of).values, asked.antibiotic.values, asked.measurement_value.values,
               asked.measurement_sign.values)
    out['inferred_rows'], out['cases_with_ranges'] = int(len(asked)), int(len(mic_ranges))

    def same(got, want):
        assert same_arrays(got, want)
    inferred, c3 = compare('infer_sir_batch', lambda c: ai.infer_sir_batch(*columns, mic_ranges, case_to_standard, ctx=c), same)
    out['inferred_classes'] = {str(k): int(v) for k, v in pd.Series(inferred[0]).value_counts(dropna=False).items()}

    # the library calls alone, on the arrays of this input
    out['tuple_group'] = {}
    for label, cols in (('org_drug', c1.args['tuple_group'][0]), ('org_drug_standard', c1.args['tuple_group'][1]),
                        ('mic_call_7_columns', c2.args['tuple_group'][1])):
        ctx.tuple_group(cols)
        t, res = timed(lambda: ctx.tuple_group(cols), args.runs + 2)
        out['tuple_group'][label] = dict(t, records=int(cols.shape[1]), columns=int(cols.shape[0]), distinct=int(res[2]),
                                         input_bytes=int(cols.nbytes), output_bytes=int(8 * cols.shape[1]))
    arrays = c3.args['mic_infer']
    ctx.mic_infer(*arrays)
    t, _ = timed(lambda: ctx.mic_infer(*arrays), args.runs + 2)
    out['mic_infer'] = dict(t, rows=int(arrays[7].size), cases=int(arrays[0].size - 1), class_entries=int(arrays[1].size),
                            fvals=int(arrays[5].size), tvals=int(arrays[6].size), row_bytes=int(sum(a.nbytes for a in arrays[7:])) +
                            4 * int(arrays[7].size))

    # per-kernel times, a run of its own
    ctx.profile(True)
    ctx.profile_reset()
    ai.extract_primary_stnds(org_to_gids, df, args.min_entries, ctx=ctx)
    ai.extract_mic_calls(org_to_gids, df, args.min_entries, ctx=ctx)
    ai.infer_sir_batch(*columns, mic_ranges, case_to_standard, ctx=ctx)
    kern = {k: {'ms': ms, 'launches': n} for k, (ms, n) in ctx.profile_read().items()}
    ctx.profile(False)
    out['kernel_ms'] = kern
    out['kernel_ms_total'] = sum(v['ms'] for v in kern.values())
    ctx.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
