"""The Bernoulli likelihood kernels (pangenomix_amd/csrc/bernoulli.hip) at every geometry of their slab split, against
tests/bernoulli_model.py's evaluate() (float64 products, longdouble logs, quotients and sums; checked against the
reference's fixtures and against 50 digits in tests/test_bernoulli_host.py).

bernoulli_model.GEOMETRY_SHAPES are the smallest tables that reach each class; test_bernoulli_host.py asserts, on
geometry()'s fields, that they do:

    G x S          a_slabs x a_span (last)   b_slabs x b_span (last)   reaches
    300 x 17       2 x 9 (8)                 5 x 1                     ragged pass A
    300 x 40       3 x 14 (12)               5 x 1                     ragged pass A, 3 slabs
    257 x 257      17 x 16 (1)               5 x 1                     last slab of one genome; two x-blocks in both passes
    64 x 1100      69 x 16 (12)              1 x 1                     one word; G + S > 1024 in the mode / total kernels
    16001 x 1025   17 x 61 (49)              126 x 2 (1)               b_span 2, ragged last slab; 1 valid bit in the last word
    52545 x 257    5 x 52 (49)               411 x 2 (2)               b_span 2, full last slab; 1 valid bit in the last word
    70001 x 400    4 x 100                   547 x 2                   a_slabs set by the wave target

Every table (random, about 10 % absent cells, one all-ones and one all-zero row) is evaluated at an interior point and
at a point with entries on both bounds, in fast mode and with PGX_BERNOULLI_EXACT, through bernoulli_load /
bernoulli_eval (the library builds the bitmap from the coordinates) and through bernoulli_eval_dev (the bitmap packed by
numpy, a guarded workspace of exactly workspace_bytes() full of garbage, both patterns). All of them give the same
bytes. Against evaluate(): bernoulli_model.assert_evaluation (LL within 1e-12 x ll_scale + 2 u x present cells, a
gradient entry within 1e-12 x its scale, specials in the same places). The two tables whose last word has one valid bit
run again with that gene present everywhere and absent everywhere."""
import numpy as np
import pytest
import torch

import bernoulli_model as bm
import dev_entry_checks as chk
from pangenomix_amd import _native

pytestmark = pytest.mark.gpu
ONE_VALID_BIT = [shape for shape in bm.GEOMETRY_SHAPES if shape[0] % 64 == 1 and shape[0] > 10000]
CASES = [shape + ('random',) for shape in bm.GEOMETRY_SHAPES] + [
    shape + (variant,) for shape in ONE_VALID_BIT for variant in ('last_gene_present', 'last_gene_absent')]


def pack_bitmap(X):
    """genome-major, gene g = bit g & 63 of word g >> 6, rows of pgx_bitmap_stride_words() words (pgx.h); pad bits zero"""
    G, S = X.shape
    stride = int(_native.lib().pgx_bitmap_stride_words(G))
    dense = np.zeros((S, stride * 64), dtype=bool)
    dense[:, :G] = X.T
    return np.packbits(dense, axis=1, bitorder='little').view('<u8')


class LoadedTable(object):
    """X on the device twice: loaded into the context from its coordinates, and as a caller's bitmap tensor."""

    def __init__(self, ctx, X):
        self.ctx, self.X, (self.G, self.S) = ctx, X, X.shape
        rows, cols = (a.astype(np.int32) for a in np.nonzero(X))
        assert ctx.bernoulli_load(rows, cols, self.G, self.S) == 0
        self.bits = chk.upload(pack_bitmap(X))
        self.nws = int(_native.lib().pgx_bernoulli_workspace_bytes(self.G, self.S))
        assert self.nws == bm.geometry(self.G, self.S).workspace_bytes

    def eval_dev(self, pq, exact, fill):
        out, ws = chk.guarded((1 + self.G + self.S) * 8, fill), chk.guarded(self.nws, fill)
        d_pq = chk.upload(pq)
        with chk.unchanged(d_pq, self.bits):
            self.ctx.bernoulli_eval_dev(self.bits.ptr, self.G, self.S, d_pq.ptr, out.ptr, ws.ptr, self.nws,
                                        1 if exact else 0, 0)
        torch.cuda.synchronize()
        out.assert_guards_intact(), ws.assert_guards_intact()
        return (out.numpy(np.float64),)

    def eval_all_entries(self, pq, exact):
        """the host entry and the device entry over both garbage patterns: one result, the same bytes from each"""
        out, = chk.same_bytes([self.eval_dev(pq, exact, fill) for fill in chk.FILLS])
        assert out.tobytes() == self.ctx.bernoulli_eval(pq, exact=exact).tobytes()
        return out


@pytest.mark.parametrize('G,S,variant', CASES, ids=['%dx%d-%s' % c for c in CASES])
def test_every_slab_geometry_matches_the_model(G, S, variant, gpu_ctx):
    rng = np.random.default_rng(G * 4099 + S)
    X = bm.random_table(rng, G, S)
    points = bm.interior_and_bounds_points(rng, G + S)
    if variant != 'random':
        X[G - 1] = variant == 'last_gene_present'           # the one gene of the last bitmap word
        del points['bounds']
    table = LoadedTable(gpu_ctx, X)
    for name, pq in points.items():
        ev = bm.evaluate(X, pq)
        assert np.isfinite(ev.ll) and np.all(np.isfinite(ev.grad))
        for exact in (False, True):
            out = table.eval_all_entries(pq, exact)
            err, bound = bm.assert_evaluation(out, ev, (name, exact))
            print('%d x %d %s %s %s: LL error %.3g (bound %.3g), gradient error / scale %.3g'
                  % (G, S, variant, name, 'exact' if exact else 'fast', err, bound,
                     float((np.abs(out[1:] - ev.grad) / ev.scale).max())))
