"""TEST INFRASTRUCTURE shared by the tests of the device-pointer entry points (pgx_*_dev): caller-owned torch tensors with
guard bands and garbage in them, inputs made on the caller's stream, no allocation inside an entry.

  guarded(nbytes, fill)   output buffers and workspaces: `nbytes` payload bytes between two bands of GUARD bytes. GUARD is
                          4096: a multiple of 256, so the payload keeps the 256-byte alignment torch's allocator gives
                          (the entries ask for 16), and wider than anything a kernel here moves per lane and step (16
                          bytes) or per wave and step (1 KiB), so an access that is off by one element, one lane or one
                          wave row lands in a band instead of in a neighbouring allocation. Bands hold 0xA5, payloads a
                          non-zero pattern of FILLS -- 0xFF (nan, -1, all-ones words) and 0x5A -- never zeros.
  upload(array)           an input produced ON THE CURRENT STREAM right before the call: a non-blocking copy from pinned
                          memory of the bytes xor 0x3C, then an in-place xor that makes the final values.
  unchanged(...)          inputs are compared byte for byte with a copy taken before the call.
  stream_scope(kind)      'null': stream 0; 'side': a torch.cuda.Stream() that is first kept busy for a while, so that work
                          an entry put on another stream would overtake the inputs. One host synchronisation, at the end.
  assert_no_allocation    free device memory is the same before and after a call (after one warm-up call, so that the
                          profiler's vectors have grown)."""
import contextlib

import numpy as np
import torch

GUARD = 4096
GUARD_BYTE = 0xA5
FILLS = (0xFF, 0x5A)
STREAMS = ('null', 'side')
_XOR = 0x3C


class Guarded(object):
    def __init__(self, nbytes, fill):
        self.nbytes = int(nbytes)
        self.raw = torch.empty(GUARD + self.nbytes + GUARD, dtype=torch.uint8, device='cuda')
        self.raw[:GUARD] = GUARD_BYTE
        self.raw[GUARD + self.nbytes:] = GUARD_BYTE
        self.raw[GUARD:GUARD + self.nbytes] = int(fill)
        self.fill = int(fill)

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def numpy(self, dtype):
        """the payload (synchronises)"""
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy().view(dtype)

    def is_still_garbage(self):
        return bool((self.raw[GUARD:GUARD + self.nbytes] == self.fill).all().item())

    def assert_guards_intact(self):
        lo, hi = self.raw[:GUARD], self.raw[GUARD + self.nbytes:]
        assert bool((lo == GUARD_BYTE).all().item()), 'bytes before the buffer were written'
        assert bool((hi == GUARD_BYTE).all().item()), 'bytes behind the buffer were written'


def guarded(nbytes, fill):
    return Guarded(nbytes, fill)


class Uploaded(object):
    """A device copy of `array`, made on the current stream."""

    def __init__(self, array):
        array = np.ascontiguousarray(array)
        host = torch.from_numpy(array.reshape(-1).view(np.uint8) ^ np.uint8(_XOR)).pin_memory()
        self.host = host                                   # (pinned memory stays until the copy has run)
        self.dev = host.to('cuda', non_blocking=True)
        self.dev.bitwise_xor_(_XOR)
        self.nbytes = array.nbytes

    @property
    def ptr(self):
        return self.dev.data_ptr() if self.nbytes else None


def upload(array):
    return Uploaded(array)


@contextlib.contextmanager
def unchanged(*inputs):
    """inputs: Uploaded objects or uint8 tensors. The copies are taken on the current stream, after the work that makes
    the inputs; the comparison (a host synchronisation) comes when the block ends."""
    tensors = [x.dev if isinstance(x, Uploaded) else x for x in inputs]
    before = [t.clone() for t in tensors]
    yield
    for t, b in zip(tensors, before):
        assert torch.equal(t, b), 'an input was written'


@contextlib.contextmanager
def on_side_stream():
    """Yields the raw stream handle of a new torch stream that is current inside the block."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # A spinning kernel ahead of everything else (torch's own test helper, a private API; bounded, not a wait on
        # anything). 40 M cycles are some 20 ms IF the counter it reads runs near 2 GHz -- not timed on gfx950. It only
        # has to outlast the host-side enqueue of the uploads and the entry (tens of microseconds each), so even a
        # counter a hundred times faster leaves it long enough.
        torch.cuda._sleep(40000000)
        yield s.cuda_stream
    torch.cuda.synchronize()


@contextlib.contextmanager
def stream_scope(kind):
    if kind == 'side':
        with on_side_stream() as handle:
            assert handle != 0
            yield handle
    else:
        assert kind == 'null'
        yield 0
        torch.cuda.synchronize()


def assert_no_allocation(call):
    """call(): the bare entry, nothing of torch in it."""
    call()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    call()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free_before


def same_bytes(results):
    """results: one tuple of numpy arrays per garbage pattern"""
    first = results[0]
    for other in results[1:]:
        assert len(other) == len(first)
        for a, b in zip(first, other):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), 'the result depends on what the buffers held before'
    return first
