"""64-bit offsets on the read side, built cheaply: chunk offsets, slice output offsets and tar
stream offsets at and above 2^32 through chacha_slice_gather_kernel, the verification's
BLAKE2b and tar_frame_kernel, without storing 4 GiB of real chunks.

read_slices runs over a device ciphertext tensor of 2^32 + 64 MiB uninitialised bytes in which
only six chunks are real (stored by the oracle); read_tar, pfscdc_store_read_tar and
pfscdc_dev_list_read_tar render windows of a stream whose first file repeats one small stored
chunk until it is longer than 2^32 bytes.  The expected bytes come from the chunks' plaintext
and tests/tar_oracle.py piece by piece (header, content as chunk[k % size], padding, trailer),
never from a whole rendered stream."""
import ctypes as C

import numpy as np
import pytest

import tar_oracle as T
from pfs_amd import _lib
from pfs_amd import chunk as pc
from pfs_amd.cdc import ChunkParams, Chunker
from stored_chunks import Stored
from test_gpu_merge import lst_of
from test_gpu_resident import dev_layout, dev_tar, entries_of, host_tar, up

pytestmark = pytest.mark.gpu

P32 = 1 << 32
MIB = 1 << 20


@pytest.fixture(scope="module")
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


def test_read_slices_of_chunks_on_both_sides_of_4gib(chunker):
    """~1,040 chunks of ~4 MiB; two real ones below 2^32, one across it, three above, the
    batch's last (odd-sized) chunk among them.  Slices of those six at several keystream
    phases, one across 2^32 itself, listed out of order, into host memory and into an
    unaligned device tensor; one slice of an unfilled chunk above 2^32 (constant bytes, no
    Ref) comes back not ok and all zeros."""
    import torch

    n = P32 + 64 * MIB
    rng = np.random.default_rng(64)
    sizes = []
    while n - sum(sizes) > 6 * MIB:
        sizes.append(int(rng.integers(4 * MIB - 300_000, 4 * MIB + 300_000)) | 1)
    if (n - sum(sizes)) % 2 == 0:
        sizes[-1] += 1
    sizes.append(n - sum(sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    nch = len(sizes)
    assert 1000 < nch < 1100 and int(offs[-1]) == n and sizes[-1] % 2 == 1
    across = int(np.searchsorted(offs, P32, side="right")) - 1
    assert offs[across] < P32 < offs[across + 1]
    real = [3, across // 2, across, across + 1, across + 7, nch - 1]
    bad = across + 3
    assert bad not in real and offs[bad] > P32

    st = Stored([sizes[k] for k in real], 640)
    ctext = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    refs = np.zeros(nch, dtype=_lib.ref_dtype())
    for j, k in enumerate(real):
        a = int(offs[k])
        ct = np.frombuffer(st.store[bytes(st.refs[j]["id"])], dtype=np.uint8)
        ctext[a:a + sizes[k]].copy_(torch.from_numpy(ct.copy()))
        refs[k] = st.refs[j]
    ctext[int(offs[bad]):int(offs[bad + 1])].fill_(0x77)

    slices = []
    for j, k in enumerate(real):
        z = sizes[k]
        for o, m in ((0, 1), (1, 63), (17, 4099), (63, 65), (64 * 1000 + 33, 70_001),
                     (z - 130_001, 130_001), (z // 2 + 5, 12_345)):
            slices.append((k, o, m))
    o = P32 - int(offs[across])  # bytes on both sides of 2^32, and the byte at it alone
    slices += [(across, o - 50_001, 100_003), (across, o, 1), (across, o - 1, 2)]
    order = rng.permutation(len(slices))
    slices = [slices[i] for i in order]
    slices.insert(len(slices) // 2, (bad, 1000, 5000))
    where = {k: j for j, k in enumerate(real)}
    want = b"".join(bytes(m) if k == bad else st.chunks[where[k]][o:o + m] for k, o, m in slices)
    total = len(want)
    is_bad = np.array([k == bad for k, _, _ in slices])

    got, cok, sok = chunker.read_slices(ctext, offs, refs, slices)
    assert cok[real].all() and not cok[bad]
    assert np.array_equal(sok, ~is_bad)
    assert got.tobytes() == want
    t = torch.full((total + 5 + 27,), 0xA5, dtype=torch.uint8, device="cuda:0")
    out, cok, sok = chunker.read_slices(ctext, offs, refs, slices, out=t[5:5 + total])
    assert cok[real].all() and not cok[bad] and np.array_equal(sok, ~is_bad)
    host = t.cpu().numpy()
    assert host[5:5 + total].tobytes() == want
    assert (host[:5] == 0xA5).all() and (host[5 + total:] == 0xA5).all()
    del ctext, t
    torch.cuda.empty_cache()


# ---- a tar stream longer than 2^32 bytes from a small batch ---------------------------------

BIG_REPEATS = 62_000


@pytest.fixture(scope="module")
def long_stream():
    """Stored chunks of 70,000, 3,000 and 12,345 bytes; the first file is 62,000 DataRefs of the
    whole first chunk (4.34e9 bytes: above 2^32, below the 8 GiB - 1 USTAR limit), a few small
    files follow.  Returns the named slices and, per file, (name, size, content(lo, hi))."""
    st = Stored([70_000, 3000, 12_345], 650)
    named = [("/big/repeated.bin", [(0, 0, 70_000)] * BIG_REPEATS),
             ("/b/one", [(1, 2999, 1)]),
             ("/b/empty", []),
             ("/b/513", [(2, 7, 513)]),
             ("/c/odd", [(1, 1, 777), (2, 100, 1000)])]
    big = np.frombuffer(st.chunks[0], dtype=np.uint8)
    pieces = [("/big/repeated.bin", 70_000 * BIG_REPEATS,
               lambda lo, hi: big[np.arange(lo, hi, dtype=np.int64) % 70_000])]
    for name, sl in named[1:]:
        body = np.frombuffer(b"".join(st.chunks[c][o:o + z] for c, o, z in sl), dtype=np.uint8)
        pieces.append((name, len(body), lambda lo, hi, body=body: body[lo:hi]))
    assert P32 < pieces[0][1] <= T.MAX_SIZE
    return st, named, pieces


def expected_window(pieces, begin, length):
    """Bytes [begin, begin + length) of the stream, piece by piece."""
    offs, total = T.layout([z for _, z, _ in pieces])
    end = min(begin + length, total)
    out = np.zeros(max(end - begin, 0), dtype=np.uint8)  # padding and the trailer are zeros
    for (name, size, content), e in zip(pieces, offs):
        lo, hi = max(begin, e), min(end, e + 512)
        if lo < hi:
            out[lo - begin:hi - begin] = np.frombuffer(T.header(name, size), np.uint8)[lo - e:hi - e]
        lo, hi = max(begin, e + 512), min(end, e + 512 + size)
        if lo < hi:
            out[lo - begin:hi - begin] = content(lo - e - 512, hi - e - 512)
    return out.tobytes(), total


def windows(total):
    """The last multiple of 512 below 2^32 for 64 KiB; the last 8 KiB plus the trailer."""
    return [(P32 - 512, 64 << 10), (total - 1024 - 8192, 8192 + 1024)]


def test_read_tar_windows_above_4gib(chunker, long_stream):
    """pfscdc_read_tar from host and device ciphertext: the window that starts at the last
    multiple of 512 below 2^32 (content at stream offsets across 2^32, from slices whose
    output offsets pass it) and the stream's end, into host memory and into an unaligned
    device tensor whose other bytes must stay."""
    import torch

    st, named, pieces = long_stream
    flat = np.array([x for _, s in named for x in s], dtype=np.int64).reshape(-1, 3)
    sl = np.zeros(len(flat), dtype=_lib.slice_dtype())
    sl["chunk"], sl["offset"], sl["size"] = flat[:, 0], flat[:, 1], flat[:, 2]
    files, at = [], 0
    for name, s in named:
        files.append((name, at, len(s)))
        at += len(s)
    _, total = T.layout([z for _, z, _ in pieces])
    assert total > P32 + (64 << 10) and total % 512 == 0
    dev = torch.from_numpy(st.ctext).to("cuda:0")
    # (a chunk no slice of the window names is not hashed: it reports its verified mark, 0)
    for (begin, length), named_chunks in zip(windows(total), ([0], [0, 1, 2])):
        want, _ = expected_window(pieces, begin, length)
        assert len(want) == length
        got, cok, nw = chunker.read_tar(st.ctext, st.offs, st.refs, files, sl, begin=begin,
                                        length=length)
        assert nw == length and cok[named_chunks].all()
        assert got.tobytes() == want, (begin, length)
        t = torch.full((length + 3 + 29,), 0xA5, dtype=torch.uint8, device="cuda:0")
        _, cok, nw = chunker.read_tar(dev, st.offs, st.refs, files, sl, begin=begin,
                                      length=length, out=t[3:3 + length])
        host = t.cpu().numpy()
        assert nw == length and cok[named_chunks].all()
        assert host[3:3 + length].tobytes() == want
        assert (host[:3] == 0xA5).all() and (host[3 + length:] == 0xA5).all()


def test_store_and_resident_list_tar_windows_above_4gib(chunker, long_stream):
    """The same list through pfscdc_store_read_tar (host list) and pfscdc_dev_list_read_tar
    (resident list): one entry of 62,000 DataRefs, layouts equal, both paths give the same
    windows, and the windows equal the expected bytes."""
    st, named, pieces = long_stream
    store = pc.ChunkStore()
    for rid, ct in st.store.items():
        store.put(rid, ct)
    entries, _ = entries_of(st, [(name, s if len(s) != BIG_REPEATS else []) for name, s in named])
    big_ref = entries_of(st, [("x", [named[0][1][0]])])[0][0].data_refs[0]
    entries[0].data_refs.extend([big_ref] * BIG_REPEATS)
    lst = lst_of(entries)
    dev = up(chunker, lst)
    rc, offs, total = dev_layout(chunker, dev)
    assert rc == 0
    cnt, ents, _, _, ndr = lst._views()
    assert cnt == len(named) and ndr == BIG_REPEATS + 4
    tf = chunker.lib.pfscdc_index_list_tar_files(lst._p)
    sizes = (C.c_uint64 * cnt)(*[ents[i].size_bytes for i in range(cnt)])
    hoffs, htotal = (C.c_uint64 * (cnt + 1))(), C.c_uint64()
    assert chunker.lib.pfscdc_tar_layout(tf, cnt, sizes, hoffs, C.byref(htotal)) == 0
    want_offs, want_total = T.layout([z for _, z, _ in pieces])
    assert (offs, total) == (list(hoffs), htotal.value) == (want_offs, want_total)
    for begin, length in windows(total):
        want, _ = expected_window(pieces, begin, length)
        rc, host, msg = host_tar(chunker, store, lst, begin, length)
        assert rc == 0, msg
        rc, got, msg = dev_tar(chunker, store, dev, begin, length)
        assert rc == 0, msg
        assert host == got, (begin, length)
        assert got == want, (begin, length)
    dev.free()
