"""GPU parity of the read path: chunk.Storage.NewReader(ctx, dataRefs).Get(w)
(the reference's src/internal/storage/chunk/storage.go:50-55, reader.go:43-79) as
pfscdc_read_slices / pfscdc_store_read: every referenced chunk verified once, only the
referenced bytes decrypted (ChaCha20 sought to the slice, transform.go:159-170).

The stored form of a chunk comes from the oracle (Ch.create_ref_id, Ch.chacha20_xor); what a
read must return comes from Ch.read_data_ref, or from plain slicing of the plaintext.  All
results are bit-exact."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from oracle import chunker as Ch
from pfs_amd import _lib
from pfs_amd import chunk as pc
from pfs_amd.cdc import ChunkParams, Chunker, synthetic_bytes
from stored_chunks import Stored

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = Ch.Params(average_bits=12, seed=1, min=2000, max=30000)  # as tests/test_gpu_refid.py


@pytest.fixture(scope="module")
def chunker():
    c = Chunker(ChunkParams(), 0)
    yield c
    c.close()


def test_every_keystream_phase_at_every_destination_alignment(chunker):
    import torch
    st = Stored([4133], 101)
    slices, pairs, cur = [], set(), 0
    for p in range(64):
        for r in range(16):
            fill = (r - cur) % 16  # brings the running output offset to r (mod 16)
            slices.append((0, (7 * p + r) % 100, fill))
            cur += fill
            off = p + 64 * ((p + r) % 61)
            assert off % 64 == p and cur % 16 == r and off + 150 <= 4133
            pairs.add((off % 64, cur % 16))
            slices.append((0, off, 150))
            cur += 150
    assert len(pairs) == 1024
    want = st.sliced(slices)
    assert len(want) == cur
    got, cok, sok = chunker.read_slices(st.ctext, st.offs, st.refs, slices)
    assert cok.all() and sok.all() and len(sok) == len(slices)
    assert got.tobytes() == want
    # an unaligned destination inside a larger buffer: not a byte outside it changes
    t = torch.full((cur + 5 + 27,), 0xA5, dtype=torch.uint8, device="cuda:0")
    dev = torch.from_numpy(st.ctext).to("cuda:0")
    out, cok, _ = chunker.read_slices(dev, st.offs, st.refs, slices, out=t[5:5 + cur])
    assert cok.all()
    host = t.cpu().numpy()
    assert host[5:5 + cur].tobytes() == want
    assert (host[:5] == 0xA5).all() and (host[5 + cur:] == 0xA5).all()


def test_size_edges_of_chunks_and_slices(chunker):
    sizes = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    st = Stored(sizes, 102)
    edge = [0, 1, 15, 16, 17, 63, 64, 65, 129]
    slices = []
    for c, n in enumerate(sizes):
        slices.append((c, 0, n))
        if n:
            slices.append((c, n - 1, 1))
        slices.append((c, n // 2, 0))
        slices += [(c, o, z) for o in edge for z in edge if o + z <= n]
    got, cok, sok = chunker.read_slices(st.ctext, st.offs, st.refs, slices)
    assert cok.all() and sok.all()
    want = st.oracle(slices)
    assert want == st.sliced(slices)
    assert got.tobytes() == want


def test_block_counter_past_65535():
    n = (4 << 20) + 200
    st = Stored([n], 103)
    slices = [(0, (1 << 22) - 7, 14),  # keystream blocks 65,535 -> 65,536
              (0, (1 << 20) + 63, 130), (0, n - 100, 100)]
    c = Chunker(ChunkParams(), 0)
    got, cok, _ = c.read_slices(st.ctext, st.offs, st.refs, slices)
    c.close()
    assert cok.all()
    assert got.tobytes() == st.oracle(slices)


def test_any_order_repeats_and_overlap_host_and_device(chunker):
    import torch
    rng = np.random.default_rng(104)
    sizes = [int(x) for x in rng.integers(1, 20_001, 8)]
    st = Stored(sizes, 104)
    slices = []
    for _ in range(500):
        c = int(rng.integers(0, 8))
        o = int(rng.integers(0, sizes[c] + 1))
        z = int(rng.integers(0, min(sizes[c] - o, 3000) + 1))
        slices.append((c, o, z))
        if rng.random() < 0.1:
            slices.append(slices[int(rng.integers(0, len(slices)))])  # an exact repeat
    slices = slices[:500]
    want = st.oracle(slices)
    got, cok, sok = chunker.read_slices(st.ctext, st.offs, st.refs, slices)
    assert cok.all() and sok.all()
    assert got.tobytes() == want
    dev = torch.from_numpy(st.ctext).to("cuda:0")
    out = torch.zeros(len(want), dtype=torch.uint8, device="cuda:0")
    res, cok, _ = chunker.read_slices(dev, st.offs, st.refs, slices, out=out)
    assert res is out and cok.all()
    assert out.cpu().numpy().tobytes() == want
    t = chunker.last_read_timings()
    assert t["verify"] > 0 and t["gather"] > 0


def test_tampered_chunk_is_zeroed_unless_marked_verified(chunker):
    rng = np.random.default_rng(105)
    sizes = [int(x) for x in rng.integers(200, 5000, 6)]
    st = Stored(sizes, 105)
    k, pos, bit = 3, 77, 0x10
    slices = []
    for c in list(range(6)) + [3, 0, 3, 5]:
        o = int(rng.integers(0, 60))
        slices.append((c, o, int(rng.integers(100, sizes[c] - o))))
    assert any(c == k and o <= pos < o + z for c, o, z in slices)
    bad = st.ctext.copy()
    bad[int(st.offs[k]) + pos] ^= bit
    got, cok, sok = chunker.read_slices(bad, st.offs, st.refs, slices)
    assert [bool(x) for x in cok] == [c != k for c in range(6)]
    assert [bool(x) for x in sok] == [c != k for c, _, _ in slices]
    at = 0
    for c, o, z in slices:
        want = bytes(z) if c == k else st.oracle([(c, o, z)])
        assert got[at:at + z].tobytes() == want, (c, o, z)
        at += z
    # marked verified (the memCache hit): no hash pass, the slice alone is decrypted
    ver = np.zeros(6, dtype=np.uint8)
    ver[k] = 1
    got, cok, sok = chunker.read_slices(bad, st.offs, st.refs, slices, verified=ver)
    assert cok.all() and sok.all()
    flipped = bytearray(st.chunks[k])
    flipped[pos] ^= bit
    want = b"".join(bytes(flipped[o:o + z]) if c == k else st.chunks[c][o:o + z]
                    for c, o, z in slices)
    assert got.tobytes() == want
    # a chunk no slice names is not hashed: it reports its mark
    _, cok, _ = chunker.read_slices(bad, st.offs, st.refs, [(0, 0, 10)], verified=ver)
    assert [bool(x) for x in cok] == [True, False, False, True, False, False]


# ------------------------------------------------------------------ write -> read, public API

def _write_files(files, store):
    st = pc.Storage(device=0, store=store)
    drs = [[] for _ in files]

    def cb(anns):
        for a in anns:
            if a.next_data_ref is not None:
                drs[a.data].append(a.next_data_ref)

    w = st.new_writer("w", cb, pc.with_rolling_hash_config(SMALL.average_bits, SMALL.seed),
                      pc.with_min_max(SMALL.min, SMALL.max))
    for i, f in enumerate(files):
        w.annotate(pc.Annotation(data=i))
        w.write(f)
    w.close()
    return st, drs


@pytest.fixture(scope="module")
def written():
    lens = [0, 1, 30_000, 700, 45_001, 0, 1500, 64, 25_000, 3]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    data = synthetic_bytes(offs, 106)
    files = [data[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(lens))]
    st, drs = _write_files(files, pc.ChunkStore())
    return files, st, drs


def test_write_then_read_through_storage(written):
    files, st, drs = written
    chunks = Ch.chunk_stream(files, SMALL, with_ref_id=True)
    ostore, odrs = {}, [[] for _ in files]
    for ch in chunks:
        rid, dek = Ch.create_ref_id(ch.data)
        ostore[rid] = Ch.chacha20_xor(dek, ch.data)
        for a in ch.annotations:
            if a.next_data_ref is not None:
                odrs[a.data].append(a.next_data_ref)
    # chunks hold several files and files span chunks
    assert any(len(d) > 1 for d in drs)
    assert len({d.ref.id for f in drs for d in f}) < sum(len(d) for d in drs)
    for i, f in enumerate(files):
        r = st.new_reader(drs[i])
        seen = []
        r.iterate(seen.append)
        assert seen == drs[i]
        got = r.get()
        assert got == f, i
        assert got == b"".join(Ch.read_data_ref(ostore, d) for d in odrs[i]), i
    every = [d for f in drs for d in f]
    assert st.new_reader(every).get() == b"".join(files)


def test_read_into_device_tensor(written):
    import torch
    files, st, drs = written
    every = [d for f in drs for d in f]
    total = sum(len(f) for f in files)
    t = torch.full((total + 9,), 0xA5, dtype=torch.uint8, device="cuda:0")
    assert st.new_reader(every).get_into(t[3:]) == total
    host = t.cpu().numpy()
    assert host[3:3 + total].tobytes() == b"".join(files)
    assert (host[:3] == 0xA5).all() and (host[3 + total:] == 0xA5).all()


def test_missing_and_tampered_chunks_raise(written):
    import torch
    files, st, drs = written
    every = [d for f in drs for d in f]
    ids = list(dict.fromkeys(d.ref.id for d in every))
    assert len(ids) >= 3
    short = pc.ChunkStore()
    for rid in ids[:-1]:
        short.put(rid, st.store.get(rid))
    with pytest.raises(KeyError):
        pc.Storage(device=0, store=short).new_reader(every).get()
    bad = pc.ChunkStore()
    for j, rid in enumerate(ids):
        ct = bytearray(st.store.get(rid))
        if j == 1:
            ct[len(ct) // 2] ^= 0x04
        bad.put(rid, bytes(ct))
    r = pc.Storage(device=0, store=bad).new_reader(every)
    with pytest.raises(_lib.PfsCdcError) as e:
        r.get()
    assert e.value.code == _lib.PFSCDC_ECORRUPT
    t = torch.full((sum(len(f) for f in files),), 0xA5, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(_lib.PfsCdcError) as e:
        r.get_into(t)
    assert e.value.code == _lib.PFSCDC_ECORRUPT
    assert (t.cpu().numpy() == 0xA5).all()  # nothing was written


# ------------------------------------------------------------------------------- plain C

def _fnv1a64(b: bytes) -> int:
    h = 0xCBF29CE484222325
    for x in b:
        h = ((h ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_plain_c_process_reads_slices_and_store(tmp_path):
    exe = str(tmp_path / "read_consumer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "read_consumer.c"),
                    "-L", libdir, "-lpfscdc", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe], check=True)
    rng = np.random.default_rng(107)
    sizes = [0, 1, 64, 700, 4133, 9001]
    st = Stored(sizes, 107)
    slices = [(c, 0, n) for c, n in enumerate(sizes)]
    for _ in range(60):
        c = int(rng.integers(1, len(sizes)))
        o = int(rng.integers(0, sizes[c] + 1))
        slices.append((c, o, int(rng.integers(0, sizes[c] - o + 1))))
    path = str(tmp_path / "chunks.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<II", len(sizes), len(slices)))
        for i, n in enumerate(sizes):
            f.write(bytes(st.refs[i]["id"]) + bytes(st.refs[i]["dek"]) + struct.pack("<Q", n))
        for c, o, z in slices:
            f.write(struct.pack("<IIQQ", c, 0, o, z))
        f.write(st.ctext.tobytes())
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=100)
    assert res.returncode == 0, res.stderr
    want = st.oracle(slices)
    header = open(os.path.join(ROOT, "include", "pfscdc.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"#define (PFSCDC_E\w+) (-\d+)", header)}
    inval = codes["PFSCDC_EINVAL"]
    assert res.stdout.splitlines() == [
        "slices %d %016x ok %s" % (len(want), _fnv1a64(want), "1" * len(sizes)),
        "store %d %016x" % (len(want), _fnv1a64(want)),
        "einval %d %d %d" % (inval, inval, inval),
        "missing %d" % codes["PFSCDC_ENOTFOUND"],
    ]
