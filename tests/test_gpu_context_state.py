"""State a context keeps survives every other entry point.

A context holds three things between calls -- the pipeline's resident bitmap (bitmap_from_clusters), the table loaded for
the Bernoulli likelihood (bernoulli_load*) and the loaded dictionary (dict_load) -- in slots of its device workspace, next
to the slots every other entry point uses for its own buffers. Two users of one slot would overwrite or, with a larger
table, free and reallocate what the other keeps: here every other host-pointer entry point runs once on the same context,
each on a table larger than the kept ones, and the kept state must come back bit for bit."""
import numpy as np
import pytest

from pangenomix_amd import _native, cluster, synth

pytestmark = pytest.mark.gpu

G_RES, S_RES = 130, 70          # the resident bitmap
G_BERN, S_BERN = 65, 3          # the Bernoulli table
G, S = 300, 75                  # every other table: more rows and more genomes than either


def coo(rng, n_rows, n_genomes, density=0.3):
    return tuple(a.astype(np.int32) for a in np.nonzero(rng.random((n_rows, n_genomes)) < density))


def strings(items):
    blob = np.frombuffer(b''.join(items), dtype=np.uint8)
    return blob, np.cumsum([0] + [len(s) for s in items]).astype(np.uint64)


def test_kept_state_survives_every_other_entry_point():
    rng = np.random.default_rng(11)
    ctx = _native.Context(0)
    try:
        # ---- the state that is kept
        r0, c0 = coo(rng, G_RES, S_RES)
        token = ctx.bitmap_from_clusters(r0, np.arange(r0.size), c0.astype(np.uint32), np.arange(S_RES), G_RES, S_RES)
        snapshot = ctx.bitmap_resident_read(token, G_RES, S_RES)
        want = np.zeros_like(snapshot)
        np.bitwise_or.at(want, (c0, r0 >> 6), np.uint64(1) << (r0 & 63).astype(np.uint64))
        assert np.array_equal(snapshot, want)

        rb, cb = coo(rng, G_BERN, S_BERN, 0.5)
        assert ctx.bernoulli_load(rb, cb, G_BERN, S_BERN) == 0
        pq = rng.uniform(0.2, 0.9, G_BERN + S_BERN)
        ll_before = ctx.bernoulli_eval(pq)
        assert np.isfinite(ll_before).all()

        keys = [b'key-%d' % (i * i) for i in range(40)]
        queries = [keys[7], b'absent', keys[39], b'', keys[0]]
        ctx.dict_load(*strings(keys))
        answer = ctx.dict_query(*strings(queries))
        assert answer.tolist() == [7, -1, 39, -1, 0]

        # ---- every other host-pointer entry point, each on a larger table
        r, c = coo(rng, G, S)
        ones = np.ones(r.size, dtype=np.int64)
        perms = np.array([rng.permutation(S) for _ in range(4)], dtype=np.int32)
        mt_key = np.random.RandomState(3).get_state()[1].astype(np.uint32)
        ctx.presence_bitmap(r, c, G, S)
        pan, _, dup = ctx.pan_core_coo(r, c, G, S, perms)
        assert dup == 0
        ctx.row_counts(r, c, G, S)
        ctx.pan_core_table(r, c, ones, G, S, 4, mt_key.copy(), 624)
        ctx.heaps_fit(pan.astype(np.float64))
        cdf = np.cumsum(np.full(400, 1.0 / 400))
        ctx.bbn_ks_sim(cdf, cdf, 50, 8, mt_key.copy(), 624)
        ctx.bbn_draws(cdf, 1000, mt_key.copy(), 624)
        concepts, dup = ctx.fcd(r, c, G, S, 3)
        assert dup == 0 and concepts['row_offsets'].size == 4
        ctx.fcd_coverage(r, c, G, S, concepts['rows'], concepts['row_offsets'], concepts['cols'], concepts['col_offsets'])
        masks = rng.integers(0, 2 ** 63, (2, 2)).astype(np.uint64)
        out, dup = ctx.assoc(r, c, G, S, masks=masks, blocks=True)
        assert dup == 0 and out['rep_row'].size > 0
        ra, ca = coo(rng, G, S)
        runs, dups = ctx.allele_runs(ra, ca, G, S, np.arange(0, G + 1, 3), gene_rows=r[r < 100], gene_genomes=c[r < 100],
                                     n_genes=100, gene_of_run=np.arange(100))
        assert dups == (0, 0) and runs['total'].size == 100
        text = rng.integers(65, 69, 5000).astype(np.uint8)
        ctx.window_scan(text, np.stack([text[i:i + 12] for i in range(0, 4800, 16)]))
        ctx.genome_sets_diff(r, c, ra, ca, G, S)
        res, off, _ = synth.protein_set('tiny').nr_arrays()
        ctx.cluster_greedy(res, off, cluster.params_from_cdhit_args({'-n': 5, '-c': 0.8}))

        # ---- the consumers of the resident bitmap read it in place
        row_map = rng.permutation(G_RES).astype(np.int32)
        ctx.pan_core_table_resident(token, G_RES, S_RES, 4, mt_key.copy(), 624)
        ctx.fcd_resident(token, row_map, None, S_RES, 3)
        ctx.assoc_resident(token, row_map, S_RES, masks=masks, blocks=True)

        # ---- nothing of it moved
        assert ctx.bitmap_resident_read(token, G_RES, S_RES).tobytes() == snapshot.tobytes()
        assert ctx.bernoulli_eval(pq).tobytes() == ll_before.tobytes()
        assert np.array_equal(ctx.dict_query(*strings(queries)), answer)
        ctx.bernoulli_load_resident(token, row_map, S_RES)
        assert ctx.bitmap_resident_read(token, G_RES, S_RES).tobytes() == snapshot.tobytes()
    finally:
        ctx.close()
