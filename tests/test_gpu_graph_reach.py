"""Shortest-path lengths from many sources to many targets on the device (csrc/reach.hip; include/pgx.h "Shortest-path
lengths") against one breadth-first search per pair (tests/reach_model.py). Integers: every comparison is
exact, and every case runs twice for equal bytes."""
import numpy as np
import pytest

import dev_entry_checks as dev
import reach_model as model
from pangenomix_amd import _native

pytestmark = pytest.mark.gpu


def check(ctx, n_nodes, edges, targets, sources):
    off, succ = model.csr(n_nodes, edges)
    want = model.lengths(off, succ, targets, sources)
    got, rounds = ctx.graph_reach(off, succ, targets, sources, return_rounds=True)
    again, rounds2 = ctx.graph_reach(off, succ, targets, sources, return_rounds=True)
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want), 'lengths differ at %r' % np.argwhere(got != want)[:10].tolist()
    assert got.tobytes() == again.tobytes() and rounds == rounds2
    assert rounds == model.rounds(off, succ, targets)
    return got, rounds


def random_edges(rng, n_nodes, degree=2.0):
    m = int(n_nodes * degree)
    return list(zip(rng.integers(0, n_nodes, m).tolist(), rng.integers(0, n_nodes, m).tolist()))


def test_a_chain_of_40_takes_40_rounds(gpu_ctx):
    edges = [(i, i + 1) for i in range(39)]
    got, rounds = check(gpu_ctx, 40, edges, [39, 0, 20], list(range(40)))
    assert rounds == 40 and got[0].tolist() == [40, 1, 21] and got[39].tolist() == [1, 0, 0]


def test_a_diamond_reports_the_shorter_route(gpu_ctx):
    # 0 -> 1 -> 5 (3 nodes) and 0 -> 2 -> 3 -> 4 -> 5 (5 nodes)
    edges = [(0, 2), (2, 3), (3, 4), (4, 5), (0, 1), (1, 5)]
    got, _ = check(gpu_ctx, 6, edges, [5], [0, 2, 1])
    assert got[:, 0].tolist() == [3, 4, 2]


def test_cycles_self_loops_and_doubled_edges(gpu_ctx):
    # a 3-cycle 0 -> 1 -> 2 -> 0 with the tail 2 -> 3 -> 4; 5 is isolated; 6 has a self-loop and a doubled edge to 4
    edges = [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (6, 6), (6, 4), (6, 4)]
    got, _ = check(gpu_ctx, 7, edges, [4, 0, 5, 6, 2], [0, 1, 2, 3, 4, 5, 6])
    assert got[0].tolist() == [5, 1, 0, 0, 3]               # from 0: 0-1-2-3-4; itself; not the isolated node; ...
    assert got[4].tolist() == [1, 0, 0, 0, 0]               # a sink as source reaches itself only
    assert got[5].tolist() == [0, 0, 1, 0, 0]               # the isolated node
    assert got[6].tolist() == [2, 0, 0, 1, 0]


def test_repeated_sources_and_targets_give_repeated_rows_and_columns(gpu_ctx):
    edges = [(0, 1), (1, 2), (3, 2)]
    got, _ = check(gpu_ctx, 4, edges, [2, 2, 0, 2], [0, 3, 0, 0])
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[0], got[3])
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 0], got[:, 3])
    assert got[0].tolist() == [3, 3, 1, 3] and got[1].tolist() == [2, 2, 0, 2]


@pytest.mark.parametrize('n_targets', (1, 63, 64, 65, 130))
def test_target_counts_around_the_word_size(n_targets, gpu_ctx):
    rng = np.random.default_rng(n_targets)
    n_nodes = 300
    targets = rng.integers(0, n_nodes, n_targets).tolist()
    sources = rng.integers(0, n_nodes, 9).tolist() + targets[:2]
    got, _ = check(gpu_ctx, n_nodes, random_edges(rng, n_nodes, 1.5), targets, sources)
    assert (got == 0).any() and (got > 2).any()


def test_a_node_with_5000_successors_next_to_nodes_with_one(gpu_ctx):
    """node 0 -> 1..5000 -> each to one of the 20 nodes behind them -> 5021 (the hub's word is made by the whole workgroup)"""
    n_nodes = 5022
    edges = [(0, v) for v in range(1, 5001)] + [(v, 5001 + v % 20) for v in range(1, 5001)]
    edges += [(5001 + j, 5021) for j in range(0, 20, 2)] + [(5021, 0)]
    targets = [5021, 5002, 4999, 0, 1] + list(range(5001, 5021)) + list(range(100, 140))
    got, _ = check(gpu_ctx, n_nodes, edges, targets, [0, 1, 5000, 5002, 5021])
    assert len(targets) == 65 and got[0, :5].tolist() == [4, 3, 2, 1, 2] and got[4, 2] == 3 and got[3, 0] == 0


@pytest.mark.parametrize('n_nodes', (1, 255, 256, 257, 5000))
def test_node_counts_around_the_block_size(n_nodes, gpu_ctx):
    rng = np.random.default_rng(n_nodes)
    targets = rng.integers(0, n_nodes, 10).tolist() + [n_nodes - 1, 0]
    sources = rng.integers(0, n_nodes, 8).tolist() + [n_nodes - 1, 0]
    check(gpu_ctx, n_nodes, random_edges(rng, n_nodes) if n_nodes > 1 else [(0, 0)], targets, sources)
    check(gpu_ctx, n_nodes, [], targets, sources)                               # no edges at all: one round


def test_nothing_to_do(gpu_ctx):
    off, succ = model.csr(3, [(0, 1)])
    assert gpu_ctx.graph_reach(off, succ, [], [0, 1]).shape == (2, 0)
    assert gpu_ctx.graph_reach(off, succ, [1], []).shape == (0, 1)
    assert gpu_ctx.graph_reach(off, succ, [1], [], return_rounds=True)[1] == 0


def test_invalid_calls_are_refused_before_anything_is_written(gpu_ctx):
    lib, P, h = _native.lib(), _native._ptr, gpu_ctx._h
    u32 = lambda *x: np.array(x, dtype=np.uint32)                                # noqa: E731
    off, succ, tgt, src = u32(0, 1, 2, 2), u32(1, 2), u32(2, 0), u32(0, 1)
    out = np.full(5, 0x6E6E6E6E, dtype=np.uint32)                                # 4 lengths and the rounds

    def refused(rc, who):
        assert rc == -1, who                                                     # PGX_ERR_INVALID
        assert (out == 0x6E6E6E6E).all(), who

    def call(off=off, succ=succ, n_nodes=3, tgt=tgt, src=src):
        return lib.pgx_graph_reach(h, P(off), P(succ), n_nodes, P(tgt), tgt.size, P(src), src.size, P(out), P(out[4:]))
    refused(call(n_nodes=1 << 24), 'n_nodes')
    refused(call(off=u32(0, 1 << 31), n_nodes=1), '2^31 edges')
    refused(call(off=u32(0, 2, 1, 2)), 'decreasing offsets')
    refused(call(off=u32(1, 1, 2, 2)), 'offsets that do not start at 0')
    refused(call(succ=u32(1, 3)), 'a successor outside the graph')
    refused(call(tgt=u32(2, 3)), 'a target outside the graph')
    refused(call(src=u32(0xFFFFFFFF, 1)), 'a source outside the graph')
    assert call() == 0 and out.tolist() == [3, 1, 2, 0, 3]
    assert lib.pgx_graph_reach_workspace_bytes(1 << 24, 1, 1) == 0
    assert lib.pgx_graph_reach_workspace_bytes(1 << 23, 64 * 32 + 1, 1) == 0     # 2^28 words and more
    assert lib.pgx_graph_reach_workspace_bytes(10, 1 << 16, 1 << 15) == 0        # 2^31 lengths
    ws_bytes = lib.pgx_graph_reach_workspace_bytes(3, 2, 2)
    assert ws_bytes >= 2 * 3 * 8 + 4
    g = dev.guarded(4096, 0x5A)
    for n_nodes, n_edges, ws in ((1 << 24, 2, 1 << 30), (3, 1 << 31, ws_bytes), (3, 2, ws_bytes - 1), (3, 2, 0)):
        with pytest.raises(_native.PgxError) as e:
            gpu_ctx.graph_reach_dev(g.ptr, g.ptr, n_nodes, n_edges, g.ptr, 2, g.ptr, 2, g.ptr, g.ptr, g.ptr, ws)
        assert e.value.status == -1
    assert g.is_still_garbage()
    g.assert_guards_intact()


# -- the device entry ------------------------------------------------------------------------------------------------------
def dev_case(seed, n_nodes, n_targets, n_sources):
    rng = np.random.default_rng(seed)
    edges = random_edges(rng, n_nodes)
    if n_nodes > 700:
        edges += [(7, v) for v in range(100, 700)]                               # one wide node
    off, succ = model.csr(n_nodes, edges)
    return off, succ, rng.integers(0, n_nodes, n_targets).astype(np.uint32), rng.integers(0, n_nodes, n_sources).astype(np.uint32)


def run_dev(ctx, case, fill, stream, want_rounds=True):
    off, succ, tgt, src = case
    ws_bytes = ctx.graph_reach_workspace_bytes(off.size - 1, tgt.size, src.size)
    assert ws_bytes > 0
    with dev.stream_scope(stream) as handle:
        d_off, d_succ, d_tgt, d_src = dev.upload(off), dev.upload(succ), dev.upload(tgt), dev.upload(src)
        out, rounds, ws = dev.guarded(4 * tgt.size * src.size, fill), dev.guarded(4, fill), dev.guarded(ws_bytes, fill)
        with dev.unchanged(d_off, d_succ, d_tgt, d_src):
            ctx.graph_reach_dev(d_off.ptr, d_succ.ptr, off.size - 1, succ.size, d_tgt.ptr, tgt.size, d_src.ptr, src.size,
                                out.ptr, rounds.ptr if want_rounds else None, ws.ptr, ws_bytes, handle)
    for buf in (out, rounds, ws):
        buf.assert_guards_intact()
    assert want_rounds or rounds.is_still_garbage()
    return out.numpy(np.uint32).reshape(src.size, tgt.size), rounds.numpy(np.uint32)


@pytest.mark.parametrize('stream', dev.STREAMS)
def test_device_entry_on_caller_tensors(stream, gpu_ctx):
    for seed, shape in ((1, (1000, 70, 12)), (2, (1, 1, 1)), (3, (257, 64, 3))):
        case = dev_case(seed, *shape)
        want = model.lengths(*case)
        per_fill = []
        for fill in dev.FILLS:                                        # outputs and the workspace pre-filled with garbage
            got = run_dev(gpu_ctx, case, fill, stream)
            assert np.array_equal(got[0], want) and got[1].tolist() == [model.rounds(case[0], case[1], case[2])]
            per_fill.append(got)
        dev.same_bytes(per_fill)
    got = run_dev(gpu_ctx, case, 0xFF, stream, want_rounds=False)
    assert np.array_equal(got[0], want)


def test_device_entry_skips_ids_that_are_not_nodes(gpu_ctx):
    """the device entry does not look at the ids: one that is no node leads nowhere, and nothing outside the buffers is
    touched"""
    off, succ = model.csr(4, [(0, 1), (1, 2), (2, 3)])
    succ = succ.copy()
    succ[1] = 0xFFFFFFF0                                                         # 1 -> nowhere
    tgt, src = np.array([3, 9, 1], dtype=np.uint32), np.array([0, 2, 4], dtype=np.uint32)
    got, _ = run_dev(gpu_ctx, (off, succ, tgt, src), 0x5A, 'null')
    assert got.tolist() == [[0, 0, 2], [2, 0, 0], [0, 0, 0]]


def test_device_entry_does_not_allocate(gpu_ctx):
    off, succ, tgt, src = dev_case(4, 1000, 70, 12)
    ws_bytes = gpu_ctx.graph_reach_workspace_bytes(off.size - 1, tgt.size, src.size)
    d_off, d_succ, d_tgt, d_src = dev.upload(off), dev.upload(succ), dev.upload(tgt), dev.upload(src)
    out, ws = dev.guarded(4 * tgt.size * src.size, 0xFF), dev.guarded(ws_bytes, 0xFF)
    dev.assert_no_allocation(lambda: gpu_ctx.graph_reach_dev(d_off.ptr, d_succ.ptr, off.size - 1, succ.size, d_tgt.ptr, tgt.size,
                                                             d_src.ptr, src.size, out.ptr, None, ws.ptr, ws_bytes))
