"""bench.py's host-side helpers that need no GPU: the cd-hit probe against a stand-in
executable that writes a known .clstr, and the launcher rules of --gpus."""
import os
import stat
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAKE = """#!/bin/sh
# stand-in for cd-hit: clusters {s0, s2} (representative s0) and {s1}
while [ $# -gt 0 ]; do case "$1" in -o) out="$2"; shift;; esac; shift; done
printf '>Cluster 0\\n0\\t30aa, >s0... *\\n1\\t28aa, >s2... at 90.00%%\\n>Cluster 1\\n0\\t29aa, >s1... *\\n' > "$out.clstr"
: > "$out"
"""


def test_cdhit_probe_compares_membership(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    res = np.frombuffer(b'A' * 30 + b'C' * 29 + b'A' * 28, dtype=np.uint8)
    off = np.array([0, 30, 59, 87], dtype=np.uint64)
    monkeypatch.setenv('PATH', str(tmp_path / 'nothing'))
    assert bench.cdhit_reference(res, off, np.array([0, 1, 0]), np.array([0, 0, 1]), str(tmp_path)) is None
    exe = tmp_path / 'bin' / 'cd-hit'
    exe.parent.mkdir()
    exe.write_text(FAKE)
    exe.chmod(exe.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv('PATH', str(exe.parent) + os.pathsep + '/usr/bin:/bin')
    same = bench.cdhit_reference(res, off, np.array([0, 1, 0]), np.array([0, 0, 1]), str(tmp_path))
    assert same['as_reference']['membership_equal'] and same['as_reference']['clusters'] == 2
    other = bench.cdhit_reference(res, off, np.array([0, 1, 1]), np.array([0, 0, 1]), str(tmp_path))
    assert not other['all_cores_unchunked']['membership_equal']
    assert other['all_cores_unchunked']['sequences_in_a_different_cluster'] == 1


def test_gpus_must_agree_with_the_launcher():
    env = dict(os.environ, WORLD_SIZE='2', RANK='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'], env=env, capture_output=True, text=True)
    assert r.returncode != 0 and 'must agree' in r.stderr


def test_steps_must_be_positive():
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], env=env, capture_output=True, text=True)
    assert r.returncode != 0 and '--steps must be at least 1' in r.stderr


def _clustered(n, seed):
    from pangenomix_amd._native import STAT_FIELDS
    rng = np.random.default_rng(seed)
    st = {k: int(x) for k, x in zip(STAT_FIELDS, rng.integers(0, 2 ** 40, len(STAT_FIELDS)))}
    return (rng.integers(-1, n, n).astype(np.int32), rng.integers(0, 9, n).astype(np.int32),
            rng.random(n).astype(np.float32), np.zeros(n, np.uint8), 1234, st)


def test_dump_outputs_writes_what_the_step_returned(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    from pangenomix_amd._native import STAT_FIELDS
    got = _clustered(1000, 0)
    pan = np.arange(24, dtype=np.int32).reshape(4, 6)
    names = bench.dump_outputs(str(tmp_path / 'out'), got, pan, pan + 1)
    assert names == ['cluster', 'core', 'identity', 'member', 'n_clusters', 'pan', 'stats', 'strand']
    z = {n: np.load(str(tmp_path / 'out' / (n + '.npy'))) for n in names}
    assert z['identity'].dtype == np.float32 and all(z[n].dtype == np.float64 for n in names if n != 'identity')
    for n, a in (('cluster', got[0]), ('member', got[1]), ('identity', got[2]), ('strand', got[3]), ('pan', pan),
                 ('core', pan + 1)):
        assert np.array_equal(z[n], a), n
    assert z['n_clusters'].tolist() == [1234]
    assert z['stats'].tolist() == [got[5][k] for k in STAT_FIELDS if k != 'sweeps']
    # one part only (--only cluster / --only pancore)
    assert bench.dump_outputs(str(tmp_path / 'p'), None, pan, pan) == ['core', 'pan']
    assert 'pan' not in bench.dump_outputs(str(tmp_path / 'c'), got, None, None)


def test_dump_outputs_keeps_a_seeded_sample_under_the_limit(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    got = _clustered(200000, 1)
    pan = np.random.default_rng(2).integers(0, 1000, (5000, 40)).astype(np.int32)
    limit = 4 << 20
    runs = []
    for d in ('a', 'b'):
        out = tmp_path / d
        names = bench.dump_outputs(str(out), got, pan, pan, limit=limit)
        assert 'sequence_index' in names and 'iteration_index' in names
        assert sum(os.path.getsize(str(out / (n + '.npy'))) for n in names) <= limit
        z = {n: np.load(str(out / (n + '.npy'))) for n in names}
        seq, it = z['sequence_index'].astype(np.int64), z['iteration_index'].astype(np.int64)
        assert 0 < seq.size < 200000 and 0 < it.size < 5000 and (np.diff(seq) > 0).all()
        assert np.array_equal(z['cluster'], got[0][seq]) and np.array_equal(z['identity'], got[2][seq])
        assert np.array_equal(z['pan'], pan[it])
        runs.append(z)
    assert all(np.array_equal(runs[0][n], runs[1][n]) for n in runs[0])
