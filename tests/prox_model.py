"""Plain-Python models of the two device steps of the proximal pangenome builders (include/pgx.h "The two device steps of the
proximal (5'/3' UTR) pangenome builders"), and a stand-in for _native.Context that runs them, so that the ctx= layer of
pangenomix_amd.pangenome can be driven without a device.

  cut    bytes slices; a reverse window is bytes.translate through the complement table, reversed; a byte outside the table
         comes out as 0 and raises the window's bad flag
  group  the reference's own bookkeeping (pangenome.py:940-960): gene -> {sequence: len(known)}"""
import numpy as np

_FROM, _TO = b'ACGTWSRYMKNacgtwsrymkn', b'TGCAWSYRKMNtgcawsyrkmn'
COMPLEMENT = bytes(_TO[_FROM.index(b)] if b in _FROM else 0 for b in range(256))
LETTERS = _FROM


def cut(text, start, length, reverse):
    """(out bytes, out_offsets uint64 [n + 1], bad uint8 [n])"""
    text = bytes(text)
    pieces, bad = [], []
    for s, n, r in zip(start, length, reverse):
        s, n = int(s), int(n)
        assert 0 <= s and s + n <= len(text)
        w = text[s:s + n]
        if r:
            w = w.translate(COMPLEMENT)[::-1]
            bad.append(1 if 0 in w else 0)          # (a window that holds a 0 byte is bad as well: 0 has no complement)
        else:
            bad.append(0)
        pieces.append(w)
    offsets = np.zeros(len(pieces) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(p) for p in pieces], dtype=np.uint64)
    return b''.join(pieces), offsets, np.array(bad, dtype=np.uint8)


def group(records, genes):
    """(first int32 [n], variant int32 [n], n_distinct) of records (a list of bytes) keyed by genes (a list of ints)"""
    known = {}                                      # gene -> {sequence: (number, index of its first record)}
    first, variant = [], []
    for i, (seq, gene) in enumerate(zip(records, genes)):
        of_gene = known.setdefault(int(gene), {})
        if seq not in of_gene:
            of_gene[seq] = (len(of_gene), i)
        variant.append(of_gene[seq][0])
        first.append(of_gene[seq][1])
    return (np.array(first, dtype=np.int32).reshape(-1), np.array(variant, dtype=np.int32).reshape(-1),
            sum(len(v) for v in known.values()))


def blob(records, lead=0):
    """(blob uint8, offsets uint64 [n + 1]) with `lead` unused bytes in front"""
    offsets = np.zeros(len(records) + 1, dtype=np.uint64)
    offsets[0] = lead
    offsets[1:] = lead + np.cumsum([len(r) for r in records], dtype=np.uint64)
    return np.frombuffer(b'\xee' * lead + b''.join(records), dtype=np.uint8), offsets


def split(blob_bytes, offsets):
    blob_bytes = bytes(blob_bytes)
    return [blob_bytes[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


class StubContext(object):
    """Context.prox_cut and Context.prox_group on the models, with the library's limits (smaller ones can be set to drive
    the fall-back of the Python layer). calls counts what was asked of it."""

    def __init__(self, max_n=1 << 24, max_bytes=1 << 32):
        self.max_n, self.max_bytes = max_n, max_bytes
        self.calls = {'prox_cut': 0, 'prox_group': 0}

    def _refuse(self, what):
        from pangenomix_amd import _native
        err = _native.PgxError('libpgx error -1: ' + what)
        err.status = -1                             # PGX_ERR_INVALID
        raise err

    def prox_cut(self, text, start, length, reverse):
        self.calls['prox_cut'] += 1
        text = bytes(text) if isinstance(text, (bytes, bytearray, memoryview)) else np.asarray(text, dtype=np.uint8).tobytes()
        start, length = np.asarray(start, dtype=np.uint64), np.asarray(length, dtype=np.uint32)
        if len(text) >= self.max_bytes or start.size >= self.max_n or int(length.sum(dtype=np.uint64)) >= self.max_bytes:
            self._refuse('pgx_prox_cut: beyond the limits')
        if start.size and ((start.astype(object) + length.astype(object)) > len(text)).any():
            self._refuse('pgx_prox_cut: a window leaves the text')
        out, offsets, bad = cut(text, start, length, reverse)
        return np.frombuffer(out, dtype=np.uint8).copy(), offsets, bad

    def prox_group(self, blob_bytes, offsets, gene, flags=0):
        self.calls['prox_group'] += 1
        offsets = np.asarray(offsets, dtype=np.uint64)
        gene = np.asarray(gene, dtype=np.int64)
        if gene.size >= self.max_n or int(offsets[-1]) >= self.max_bytes or (gene.size and (gene.min() < 0 or gene.max() >= 1 << 24)):
            self._refuse('pgx_prox_group: beyond the limits')
        data = blob_bytes if isinstance(blob_bytes, (bytes, bytearray)) else np.asarray(blob_bytes, dtype=np.uint8).tobytes()
        return group(split(data, offsets), gene.tolist())


# -- driving pangenomix_amd.pangenome with ctx= against what the reference recorded (tests/golden/proximal_device) --------------
def recorded_runs(golden_dir):
    import json
    import os
    return json.load(open(os.path.join(golden_dir, 'proximal_device', 'expected', 'runs.json')))


def tree(root):
    """{relative path: bytes} of every file under root"""
    import os
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), 'rb') as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def expected_counts(run):
    """the PROXIMAL_PATH_COUNTS a recorded run must leave: exactly the genomes listed under 'host' go to the host, the
    hand-made extracts are not extracted at all, and a run stops at the genome the reference raised on"""
    want = {}
    for g in run['genomes']:
        if g in run.get('pre', []):
            continue
        key = 'extract_host' if g in run['host'] else 'extract_device'
        want[key] = want.get(key, 0) + 1
        if run['raised'] and g in run['host']:
            return want
    want['consolidate_device'] = 1
    return want


def run_recorded(run, ctx, tmp_path, golden_dir, capsys, all_by_the_host=False):
    """One recorded run through the ctx= layer: stdout, exception, every file byte for byte (.npz member by member), the path
    counts; then, for a run that went through, a second call on the extracts the first one left. all_by_the_host: the
    context refuses everything, so every genome and the grouping must be counted on the host side."""
    import os
    import shutil
    from pangenomix_amd import pangenome as pg
    from test_host_golden import assert_same_npz
    din = str(tmp_path / 'in')
    shutil.copytree(os.path.join(golden_dir, 'proximal_device', 'in'), din)
    out = str(tmp_path / 'out')
    os.makedirs(out)
    os.makedirs(os.path.join(din, 'derived'))
    for g in run.get('pre', []):
        shutil.copy(os.path.join(din, 'pre', '%s_%s.fna' % (g, run['side'])), os.path.join(din, 'derived'))
    fn = pg.build_upstream_pangenome if run['side'] == 'upstream' else pg.build_downstream_pangenome
    pairs = [(os.path.join(din, g + '.gff'), os.path.join(din, g + '.fna')) for g in run['genomes']]
    kw = dict(run['kw'], limits=tuple(run['kw']['limits']))
    capsys.readouterr()
    pg.PROXIMAL_PATH_COUNTS.clear()
    raised, df = None, None
    try:
        df = fn(pairs, os.path.join(din, 'T_allele_names.tsv'), out, ctx=ctx, **kw)
    except Exception as e:                          # noqa: BLE001 -- compared with what the reference raised
        raised = [type(e).__name__, [str(a) for a in e.args]]
    assert capsys.readouterr().out.replace(din, '<in>').replace(out, '<out>') == run['stdout']
    assert raised == run['raised']
    grouped = 'consolidate_host' if all_by_the_host else 'consolidate_device'
    assert dict(pg.PROXIMAL_PATH_COUNTS) == ({'extract_host': len(run['genomes']), grouped: 1} if all_by_the_host
                                             else expected_counts(run))
    exp = os.path.join(golden_dir, 'proximal_device', 'expected')
    tag = [t for t, r in recorded_runs(golden_dir).items() if r == run][0]
    got = dict(tree(out), **tree(os.path.join(din, 'derived')))
    assert sorted(got) == run['files']
    for name in run['files']:
        if name.endswith('.npz'):
            assert_same_npz(os.path.join(out, name), os.path.join(exp, tag, name))
        else:
            with open(os.path.join(exp, tag, name), 'rb') as f:
                assert got[name] == f.read(), name
    if raised is None:
        pg.PROXIMAL_PATH_COUNTS.clear()
        df2 = fn(pairs, os.path.join(din, 'T_allele_names.tsv'), out, ctx=ctx, **kw)
        assert capsys.readouterr().out.count('Using pre-existing') == len(run['genomes'])
        assert dict(pg.PROXIMAL_PATH_COUNTS) == {grouped: 1}
        assert list(df2.index) == list(df.index) and list(df2.columns) == list(df.columns)
        assert df2.data.row.tolist() == df.data.row.tolist() and df2.data.col.tolist() == df.data.col.tolist()
        again = dict(tree(out), **tree(os.path.join(din, 'derived')))
        assert {k: v for k, v in again.items() if not k.endswith('.npz')} == {k: v for k, v in got.items() if not k.endswith('.npz')}
    return df


def write_random_genomes(root, seed, n_genomes=6, n_features=300):
    """n_genomes mutated copies of one random genome (3 contigs, both strands, lower case and ambiguity codes, paralogs,
    unmapped and non-CDS lines) under root; returns (pairs, allele names path)"""
    import os
    rng = np.random.default_rng(seed)
    os.makedirs(root)
    alphabet = np.frombuffer(b'ACGT' * 12 + b'acgtNnRYKMSWrykmsw', dtype=np.uint8)
    lengths = {'k1': 9000, 'k2': 5000, 'k3': 700}
    base = {c: alphabet[rng.integers(0, alphabet.size, n)].copy() for c, n in lengths.items()}
    feats, seen = [], set()
    while len(feats) < n_features:
        c = ('k1', 'k2', 'k3')[int(rng.choice(3, p=(0.6, 0.35, 0.05)))]
        a = int(rng.integers(1, lengths[c] - 10))
        b = min(a + int(rng.integers(5, 120)), lengths[c])
        strand = '+-'[int(rng.integers(0, 2))]
        if (c, strand, a, b) in seen:
            continue
        seen.add((c, strand, a, b))
        feats.append((c, a, b, strand))
    feats.sort(key=lambda f: (f[0], f[1]))
    pairs, names = [], {}
    for gi in range(n_genomes):
        g = 'r%d' % (gi * 7 % 11)
        contigs = {c: s.copy() for c, s in base.items()}
        for c in contigs:
            at = rng.integers(0, contigs[c].size, contigs[c].size // 150)
            contigs[c][at] = alphabet[rng.integers(0, 48, at.size)]
        with open(os.path.join(root, g + '.fna'), 'w') as f:
            for c, s in contigs.items():
                s = s.tobytes().decode()
                f.write('>%s extra words\n%s\n' % (c, '\n'.join(s[i:i + 80] for i in range(0, len(s), 80))))
        with open(os.path.join(root, g + '.gff'), 'w') as f:
            f.write('##gff-version 3\n# a comment\twith a tab\n\n')
            for k, (c, a, b, strand) in enumerate(feats):
                kind = 'tRNA' if k % 41 == 40 else 'CDS'
                fid = 'fig|%s.%s.%d' % (g, 'rna' if kind == 'tRNA' else 'peg', k)
                f.write('\t'.join(['accn|' + c, 'PATRIC', kind, str(a), str(b), '.', strand, '0',
                                   'Name=n%d;ID=%s;product=x y' % (k, fid) if k % 50 == 7 else 'ID=%s;locus_tag=L%d' % (fid, k)]) + '\n')
                if kind == 'CDS' and k % 23 != 5:
                    names.setdefault(k % 120, []).append('%s|x' % fid)
        pairs.append((os.path.join(root, g + '.gff'), os.path.join(root, g + '.fna')))
    path = os.path.join(root, 'R_allele_names.tsv')
    with open(path, 'w') as f:
        for gene, heads in sorted(names.items()):
            f.write('R_C%dA0\t%s\n' % (gene, '\t'.join(heads)))
    return pairs, path


RANDOM_RUNS = (('upstream', dict(limits=(-50, 3))), ('upstream', dict(limits=(-50, 3), max_overlap=5, include_fragments=True)),
               ('downstream', dict(limits=(-3, 50), max_overlap=0)))


def compare_with_host_path(ctx, tmp_path, capsys, seed=2026):
    """the builders on generated genomes, ctx= against ctx=None: stdout, every file, the table returned"""
    import shutil
    from pangenomix_amd import pangenome as pg
    pairs, names = write_random_genomes(str(tmp_path / 'src'), seed)
    for side, kw in RANDOM_RUNS:
        results = []
        for which in (None, ctx):
            work = str(tmp_path / ('work_%s' % ('host' if which is None else 'ctx')))
            shutil.rmtree(work, ignore_errors=True)
            shutil.copytree(str(tmp_path / 'src'), work + '/in')
            local = [(a.replace(str(tmp_path / 'src'), work + '/in'), b.replace(str(tmp_path / 'src'), work + '/in')) for a, b in pairs]
            fn = pg.build_upstream_pangenome if side == 'upstream' else pg.build_downstream_pangenome
            capsys.readouterr()
            pg.PROXIMAL_PATH_COUNTS.clear()
            df = fn(local, work + '/in/R_allele_names.tsv', work, name='R', ctx=which, **kw)
            printed = capsys.readouterr().out.replace(work, '<work>')
            counts = dict(pg.PROXIMAL_PATH_COUNTS)
            files = tree(work)
            npz = {k: files.pop(k) for k in list(files) if k.endswith('.npz')}
            results.append((printed, files, sorted(npz), list(df.index), list(df.columns), df.data.row.tolist(),
                            df.data.col.tolist(), df.data.data.tolist()))
        assert counts == {'extract_device': len(pairs), 'consolidate_device': 1}, (side, kw, counts)
        for a, b in zip(*results):
            assert a == b, (side, kw)
        assert len(results[0][3]) > 100 and any('U1' in x or 'D1' in x for x in results[0][3])
