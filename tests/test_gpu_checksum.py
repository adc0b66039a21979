"""gn_checksum_device against its definition (include/gpu_nnue.h), restated in numpy.

The checksum decides equality in about ten tests, in bench.py's comparison of every timed record
with the plain path, and in the library's own depth-2 check: a kernel that dropped the tail word,
or stopped after its first grid stride, would weaken all of them unnoticed.  The sizes sit on
either side of a word, of a 256-thread block and of the first grid stride (8,192 blocks x 256
threads = 2,097,152 words = 16 MiB), and one spans more than three strides."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
MIB = 1 << 20
STRIDE = 8192 * 256 * 8  # bytes covered by one pass of the largest grid
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
SIZES = [0, 1, 7, 8, 9, 24, 24 * 1000, 8 * 255, 8 * 256, 8 * 257,
         16 * MIB - 8, 16 * MIB, 16 * MIB + 8, 16 * MIB + 13, 48 * MIB + 5]
OFFSETS = (0, 8, 4096)
assert STRIDE == 16 * MIB


def mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def checksum(data: np.ndarray) -> int:
    """sum over the little-endian 64-bit words w_i (the tail zero-padded) of mix(w_i ^ i * golden),
    modulo 2^64; 0 for no bytes."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    padded = np.zeros((len(data) + 7) // 8 * 8, dtype=np.uint8)
    padded[:len(data)] = data
    w = padded.view("<u8")
    with np.errstate(over="ignore"):
        i = np.arange(len(w), dtype=np.uint64)
        return int(mix(w ^ (i * GOLDEN)).sum(dtype=np.uint64))


def test_the_restatement_itself():
    """Against Python integers, on words small enough to follow by hand."""
    M = (1 << 64) - 1

    def mix_int(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    data = bytes(range(1, 20))  # two words and a tail of three bytes
    words = [int.from_bytes(data[k:k + 8].ljust(8, b"\0"), "little") for k in range(0, len(data), 8)]
    want = sum(mix_int(w ^ (i * 0x9E3779B97F4A7C15 & M)) for i, w in enumerate(words)) & M
    assert checksum(np.frombuffer(data, dtype=np.uint8)) == want
    assert checksum(np.zeros(0, dtype=np.uint8)) == 0
    assert checksum(np.zeros(8, dtype=np.uint8)) == 0 and checksum(np.zeros(16, dtype=np.uint8)) == mix_int(0x9E3779B97F4A7C15)


@pytest.fixture(scope="module")
def uploaded(gpu_ctx):
    """48 MiB + 4 KiB + 16 seeded random bytes on the device, and on the host."""
    n = max(SIZES) + max(OFFSETS) + 16
    data = np.random.default_rng(0x5EEDC5).integers(0, 256, n, dtype=np.uint8)
    buf = gpu_ctx.alloc(n)
    assert buf.addr % 8 == 0
    buf.upload(data)
    yield buf, data
    buf.free()


@gpu
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("size", SIZES)
def test_checksum_equals_its_definition(gpu_ctx, uploaded, size, offset):
    buf, data = uploaded
    assert gpu_ctx.checksum_device(buf, size, offset) == checksum(data[offset:offset + size])


@gpu
def test_all_zero_buffer(gpu_ctx):
    n = 16 * MIB + 8
    zeros = np.zeros(n, dtype=np.uint8)
    buf = gpu_ctx.alloc(n)
    try:
        buf.upload(zeros)
        got = gpu_ctx.checksum_device(buf, n)
        assert got == checksum(zeros) != 0  # the position term alone: mix(i * golden) over the words
        assert gpu_ctx.checksum_device(buf, 8) == 0 == checksum(zeros[:8])
    finally:
        buf.free()


def _patched(gpu_ctx, buf, data, edits):
    """The device checksum after writing edits {byte index: value} into the device copy; restores it."""
    n = len(data)
    changed = data.copy()
    for k, v in edits.items():
        changed[k] = v
    words = sorted({k // 8 for k in edits})
    try:
        for w in words:
            lo, hi = 8 * w, min(8 * w + 8, n)
            _upload_at(gpu_ctx, buf, lo, changed[lo:hi])
        return gpu_ctx.checksum_device(buf, n), checksum(changed)
    finally:
        for w in words:
            lo, hi = 8 * w, min(8 * w + 8, n)
            _upload_at(gpu_ctx, buf, lo, data[lo:hi])


def _upload_at(ctx, buf, offset, arr):
    from fishnet_amd import gpu_nnue as G
    a = np.ascontiguousarray(arr)
    assert offset + a.nbytes <= buf.nbytes
    G._check(G.lib().gn_memcpy_h2d(ctx.h, buf.slot, C.c_void_p(buf.addr + offset), a.ctypes.data, a.nbytes))


@pytest.fixture(scope="module")
def two_strides(gpu_ctx):
    """16 MiB + 8 KiB + 13 bytes: a full first stride, 1,024 words of the second and a tail."""
    n = STRIDE + 8192 + 13
    data = np.random.default_rng(0x5EEDC6).integers(0, 256, n, dtype=np.uint8)
    buf = gpu_ctx.alloc(n)
    buf.upload(data)
    yield buf, data, gpu_ctx.checksum_device(buf, n)
    buf.free()


@gpu
@pytest.mark.parametrize("where", ("first word", "first word of the second stride", "tail"))
def test_a_changed_byte_changes_the_sum(gpu_ctx, two_strides, where):
    buf, data, before = two_strides
    assert before == checksum(data)
    k = {"first word": 3, "first word of the second stride": STRIDE + 5, "tail": len(data) - 1}[where]
    got, want = _patched(gpu_ctx, buf, data, {k: int(data[k]) ^ 0x40})
    assert got == want != before
    assert gpu_ctx.checksum_device(buf, len(data)) == before  # restored


@gpu
def test_words_swapped_across_the_stride_boundary(gpu_ctx, two_strides):
    """The last word of the first stride and the first of the second go to the same thread in
    successive passes: swapped, they change the sum through the position term alone."""
    buf, data, before = two_strides
    a, b = data[STRIDE - 8:STRIDE].copy(), data[STRIDE:STRIDE + 8].copy()
    assert a.tobytes() != b.tobytes()
    edits = {STRIDE - 8 + k: int(b[k]) for k in range(8)}
    edits.update({STRIDE + k: int(a[k]) for k in range(8)})
    got, want = _patched(gpu_ctx, buf, data, edits)
    assert got == want != before


@gpu
def test_misaligned_pointer_is_rejected_before_any_launch(gpu_ctx, uploaded):
    """d_ptr not 8-byte aligned: GN_E_INVALID from the host-side argument check.  *sum stays as it was
    (a launch would have been followed by its store), and the next call still works."""
    from fishnet_amd import gpu_nnue as G
    buf, data = uploaded
    for off in (1, 2, 4, 7, 4097):
        v = C.c_uint64(0xDEADBEEF)
        rc = G.lib().gn_checksum_device(gpu_ctx.h, 0, C.c_void_p(buf.addr + off), 64, C.byref(v))
        assert rc == G.E_INVALID and v.value == 0xDEADBEEF
        assert b"aligned" in G.lib().gn_last_error()
        with pytest.raises(G.GnError) as e:
            gpu_ctx.checksum_device(buf, 64, off)
        assert e.value.code == G.E_INVALID
    assert gpu_ctx.checksum_device(buf, 64, 8) == checksum(data[8:72])
