#!/usr/bin/env python
"""Timing of MLST typing and of the pattern scan under it. Prints one JSON object.

    python tools/mlst_bench.py [--runs 5] [--genomes 16] [--out profiles/mlst_bench.json]
    python tools/mlst_bench.py --near-only --near-out profiles/mlst_near_bench.json      

The input is synthetic (pangenomix_amd.synth): a genome of --bases (5 Mbp) of random ACGT in --contigs (50) contigs that carries
one allele of every locus, half of them on the minus strand, and two schemes of 7 loci x 450 bases, one of 300 and one of
3,000 alleles per locus (point mutants of one ancestor per locus, so most alleles of a locus share their seed). Per scheme,
median / min / max of --runs runs after a warm-up, in one process on one machine:
  pattern_load, pattern_query   the two library calls with their transfers
  kernel_ms                     per-kernel time of ONE profiled load + query (pgx_profile_read; a run of its own)
  yardstick                     scan_kernel (csrc/scan.hip) on the same text with
                                window = seed and as many keys as the patterns have distinct seeds: the same per-position work
                                without any verification; ratio = pattern_scan_kernel / scan_kernel
  call_alleles                  per genome over --genomes copies of the genome file (links to one file; each is read and parsed
                                again), with ctx and with ctx=None

--near-out adds the novel-allele leg on the 7 x 300 x 450 scheme and writes it to a file of its own: the same genome with one
and with three loci made novel by one substitution; per variant
  near_load, near_query         the two library calls with their transfers (all patterns loaded, m = 22, blocks of 19; the query
                                with the patterns of the novel loci active, as call_alleles asks it), checked against host_near
  kernel_ms                     per-kernel time of ONE profiled load + query
  yardstick                     pattern_scan_kernel (csrc/pattern.hip) on the same text and scheme in the same process; ratio =
                                near_scan_kernel / pattern_scan_kernel
  call_alleles                  per genome with min_identity=95, with ctx (--genomes copies) and ctx=None (--near-host-genomes)
and, on the genome without a novel locus, call_alleles with min_identity=None per genome, --runs runs with their spread, beside
the figure the parent commit recorded in profiles/mlst_bench.json: the check that the default path did not get slower.
"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pangenomix_amd import _native, mlst, synth           # noqa: E402


def timed(fn, runs):
    fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return {'median': float(np.median(t)), 'min': min(t), 'max': max(t)}, out


def note(*words):
    print(*words, file=sys.stderr, flush=True)


@contextlib.contextmanager
def heartbeat(what, every=60.0):
    """a line on stderr every `every` seconds while the block runs"""
    done = threading.Event()

    def run():
        t0 = time.perf_counter()
        while not done.wait(every):
            note('... %s: %.0f s so far' % (what, time.perf_counter() - t0))
    thread = threading.Thread(target=run, daemon=True)
    thread.start()
    try:
        yield
    finally:
        done.set()
        thread.join()


def profiled(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    fn()
    kern = {k: {'ms': ms, 'launches': n} for k, (ms, n) in ctx.profile_read().items()}
    ctx.profile(False)
    return kern


def near_leg(ctx, args, tmp):
    """the novel-allele leg (see the module's docstring); returns its record"""
    scheme = synth.mlst_scheme(n_loci=7, n_alleles=300, length=450, seed=21)
    key, st = next(iter(scheme.profiles.items()))
    carried = {locus: (number, '+-'[i % 2]) for i, (locus, number) in enumerate(zip(scheme.loci, key))}
    pats = mlst._Patterns(scheme)
    near_m = [mlst.max_mismatches(len(p), 95) for p in pats.patterns]
    block = min([mlst.MAX_BLOCK] + [len(p) // (m + 1) for p, m in zip(pats.patterns, near_m)])
    out = {'device': ctx.device_info()['name'], 'runs': args.runs, 'genomes': args.genomes, 'host_genomes': args.near_host_genomes,
           'bases': args.bases, 'contigs': args.contigs, 'scheme': '7x300x450', 'min_identity': 95, 'patterns': len(pats.patterns),
           'max_mismatch': max(near_m), 'block': block, 'table_entries': int(sum(near_m) + len(near_m)), 'variants': {}}

    def copies(first, n, tag):
        paths = [first]
        for g in range(1, n):
            paths.append(os.path.join(tmp, '%s_%d.fna' % (tag, g)))
            os.symlink(first, paths[-1])
        return paths
    for tag, novel in (('one_novel_locus', (scheme.loci[4],)), ('three_novel_loci', (scheme.loci[1], scheme.loci[4], scheme.loci[6]))):
        first = synth.mlst_genome(scheme, os.path.join(tmp, tag + '_0.fna'), carried, n_bp=args.bases, n_contigs=args.contigs,
                                  seed=3, novel=novel)
        paths = copies(first, args.genomes, tag)
        text = b'\x00'.join(mlst.read_genome(first)[1])
        active = np.zeros(len(pats.patterns), dtype=np.uint8)
        for li, number, seq, fwd, rev in pats.rows:
            if scheme.loci[li] in novel:
                active[fwd] = active[rev] = 1
        rec = {'novel_loci': len(novel), 'active_patterns': int(active.sum()), 'text_bytes': len(text)}
        rec['near_load'], _ = timed(lambda: ctx.near_load(pats.blob, pats.offsets, near_m, block), args.runs)
        rec['near_query'], best = timed(lambda: ctx.near_query(text, separator=0, active=active), args.runs)
        with heartbeat('host_near'):
            want = mlst.host_near(text, pats.patterns, near_m, block, separator=0, active=active)
        assert np.array_equal(best, want) and int((best != mlst.NEAR_NONE).sum()) >= len(novel)
        rec['patterns_within_threshold'] = int((best != mlst.NEAR_NONE).sum())
        kern = profiled(ctx, lambda: (ctx.near_load(pats.blob, pats.offsets, near_m, block),
                                      ctx.near_query(text, separator=0, active=active)))
        rec['kernel_ms'] = kern
        rec['pattern_load'], _ = timed(lambda: ctx.pattern_load(pats.blob, pats.offsets, seed=pats.seed), args.runs)
        rec['pattern_query'], _ = timed(lambda: ctx.pattern_query(text), args.runs)
        base = profiled(ctx, lambda: (ctx.pattern_load(pats.blob, pats.offsets, seed=pats.seed), ctx.pattern_query(text)))
        a, b = kern.get('near_scan_kernel', {}).get('ms', 0), base.get('pattern_scan_kernel', {}).get('ms', 0)
        rec['yardstick'] = {'what': 'pattern_scan_kernel of csrc/pattern.hip on the same text and scheme, seed 32', 'kernel_ms': base,
                            'near_scan_kernel_ms': a, 'pattern_scan_kernel_ms': b, 'ratio': a / b if b > 0 else None}
        note(tag, 'library calls and kernels timed, ratio', rec['yardstick']['ratio'])
        mlst.call_alleles(scheme, paths[:2], ctx=ctx, min_identity=95)                               # warm-up
        t0 = time.perf_counter()
        frame = mlst.call_alleles(scheme, paths, ctx=ctx, min_identity=95)
        dev_s = time.perf_counter() - t0
        with heartbeat('call_alleles with ctx=None'):
            t0 = time.perf_counter()
            host_frame = mlst.call_alleles(scheme, paths[:args.near_host_genomes], min_identity=95)
            host_s = time.perf_counter() - t0
        assert frame.iloc[:args.near_host_genomes].equals(host_frame) and (frame['ST'] == '-').all()
        assert all(frame[locus].str.startswith('~').all() == (locus in novel) for locus in scheme.loci)
        rec['call_alleles'] = {'ctx_seconds_per_genome': dev_s / args.genomes,
                               'host_seconds_per_genome': host_s / args.near_host_genomes,
                               'host_over_ctx': (host_s / args.near_host_genomes) / (dev_s / args.genomes)}
        note(tag, 'call_alleles per genome: %.4f s with ctx, %.3f s without' % (dev_s / args.genomes, host_s / args.near_host_genomes))
        out['variants'][tag] = rec
    # the default path, on the genome the exact benchmark uses
    first = synth.mlst_genome(scheme, os.path.join(tmp, 'plain_0.fna'), carried, n_bp=args.bases, n_contigs=args.contigs, seed=3)
    paths = copies(first, args.genomes, 'plain')
    mlst.call_alleles(scheme, paths[:2], ctx=ctx)                                                    # warm-up
    per_genome = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        frame = mlst.call_alleles(scheme, paths, ctx=ctx)
        per_genome.append((time.perf_counter() - t0) / args.genomes)
    assert (frame['ST'] == st).all()
    rec = {'ctx_seconds_per_genome': {'median': float(np.median(per_genome)), 'min': min(per_genome), 'max': max(per_genome)},
           'runs': per_genome}
    try:
        with open(os.path.join(ROOT, 'profiles', 'mlst_bench.json')) as f:
            rec['parent_commit_ctx_seconds_per_genome'] = json.load(f)['schemes']['7x300x450']['call_alleles']['ctx_seconds_per_genome']
    except (OSError, KeyError, ValueError):
        rec['parent_commit_ctx_seconds_per_genome'] = None
    t0 = time.perf_counter()
    frame95 = mlst.call_alleles(scheme, paths, ctx=ctx, min_identity=95)
    rec['ctx_seconds_per_genome_with_min_identity_95'] = (time.perf_counter() - t0) / args.genomes
    assert frame95.equals(frame)
    out['call_alleles_min_identity_none'] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--near-out', default=None, help='run the novel-allele leg and write its record here')
    ap.add_argument('--near-only', action='store_true', help='skip the exact-scan legs')
    ap.add_argument('--near-host-genomes', type=int, default=1)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--genomes', type=int, default=16)
    ap.add_argument('--bases', type=int, default=5000000)
    ap.add_argument('--contigs', type=int, default=50)
    ap.add_argument('--alleles', type=int, nargs='+', default=[300, 3000])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    ctx = _native.Context(0)
    out = {'device': ctx.device_info()['name'], 'runs': args.runs, 'genomes': args.genomes, 'bases': args.bases,
           'contigs': args.contigs, 'schemes': {}}
    with tempfile.TemporaryDirectory() as tmp:
        if args.near_out:
            near = near_leg(ctx, args, tmp)
            with open(args.near_out, 'w') as f:
                f.write(json.dumps(near, indent=1, sort_keys=True) + '\n')
            out['near'] = near
        for n_alleles in ([] if args.near_only else args.alleles):
            scheme = synth.mlst_scheme(n_loci=7, n_alleles=n_alleles, length=450, seed=21)
            key, st = next(iter(scheme.profiles.items()))
            carried = {locus: (number, '+-'[i % 2]) for i, (locus, number) in enumerate(zip(scheme.loci, key))}
            first = synth.mlst_genome(scheme, os.path.join(tmp, 'g%d_0.fna' % n_alleles), carried, n_bp=args.bases,
                                      n_contigs=args.contigs, seed=3)
            paths = [first]
            for g in range(1, args.genomes):
                paths.append(os.path.join(tmp, 'g%d_%d.fna' % (n_alleles, g)))
                os.symlink(first, paths[-1])
            note('scheme 7 x %d x 450: files written' % n_alleles)
            pats = mlst._Patterns(scheme)
            text = b'\x00'.join(mlst.read_genome(first)[1])
            seeds = sorted({p[:pats.seed] for p in pats.patterns})
            rec = {'patterns': len(pats.patterns), 'pattern_bytes': int(pats.blob.size), 'seed': pats.seed,
                   'distinct_seeds': len(seeds), 'text_bytes': len(text)}
            rec['pattern_load'], _ = timed(lambda: ctx.pattern_load(pats.blob, pats.offsets, seed=pats.seed), args.runs)
            rec['pattern_query'], (hit_first, hit_count) = timed(lambda: ctx.pattern_query(text), args.runs)
            want = mlst.host_scan(text, pats.patterns, pats.seed)
            assert np.array_equal(hit_first, want[0]) and np.array_equal(hit_count, want[1]) and int(hit_count.sum()) == 7
            kern = profiled(ctx, lambda: (ctx.pattern_load(pats.blob, pats.offsets, seed=pats.seed), ctx.pattern_query(text)))
            rec['kernel_ms'] = kern
            keys = np.frombuffer(b''.join(seeds), dtype=np.uint8).reshape(len(seeds), pats.seed)
            rec['window_scan'], found = timed(lambda: ctx.window_scan(text, keys), args.runs)
            base = profiled(ctx, lambda: ctx.window_scan(text, keys))
            a, b = kern.get('pattern_scan_kernel', {}).get('ms', 0), base.get('scan_kernel', {}).get('ms', 0)
            rec['yardstick'] = {'what': 'scan_kernel of csrc/scan.hip on the same text, window = seed, keys = the distinct seeds',
                                'keys': len(seeds), 'keys_found': int(found.sum()), 'kernel_ms': base,
                                'pattern_scan_kernel_ms': a, 'scan_kernel_ms': b, 'ratio': a / b if b > 0 else None}
            note('library calls and kernels timed, ratio', rec['yardstick']['ratio'])
            mlst.MLST_PATH_COUNTS.clear()
            mlst.call_alleles(scheme, paths[:2], ctx=ctx)                                            # warm-up
            t0 = time.perf_counter()
            frame = mlst.call_alleles(scheme, paths, ctx=ctx)
            dev_s = time.perf_counter() - t0
            note('call_alleles with ctx: %.3f s for %d genomes' % (dev_s, args.genomes))
            with heartbeat('call_alleles with ctx=None'):                        # minutes of host work at 3,000 alleles
                t0 = time.perf_counter()
                host_frame = mlst.call_alleles(scheme, paths)
                host_s = time.perf_counter() - t0
            note('call_alleles with ctx=None: %.3f s' % host_s)
            assert frame.equals(host_frame) and (frame['ST'] == st).all()
            assert mlst.MLST_PATH_COUNTS == {'device': args.genomes + 2, 'host': args.genomes}
            rec['read_genome'], _ = timed(lambda: mlst.read_genome(first), args.runs)
            rec['call_alleles'] = {'ctx_seconds_per_genome': dev_s / args.genomes, 'host_seconds_per_genome': host_s / args.genomes,
                                   'host_over_ctx': host_s / dev_s}
            out['schemes']['7x%dx450' % n_alleles] = rec
    ctx.close()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
