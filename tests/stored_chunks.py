"""Chunks in their stored form, shared by the GPU read-path and steady-state tests: what
chunk.Create(CreateOptions{}) uploads for each chunk, from the oracle (Ch.create_ref_id,
Ch.chacha20_xor).  The oracle runs once per distinct content: a list that repeats a content
(or two lists over the same contents in another order) pays for it once."""
import numpy as np

from oracle import chunker as Ch
from pfs_amd import _lib
from pfs_amd.cdc import synthetic_bytes

_CREATED = {}  # content -> (Ref.Id, Ref.Dek, ciphertext, content hash)


def created(chunk: bytes):
    """(id, dek, ciphertext, BLAKE2b-256(chunk)) of one chunk, from the oracle."""
    got = _CREATED.get(chunk)
    if got is None:
        rid, dek = Ch.create_ref_id(chunk)
        got = _CREATED[chunk] = (rid, dek, Ch.chacha20_xor(dek, chunk), Ch.blake2b256(chunk))
    return got


class Stored:
    """A batch of chunks as chunk.Create(CreateOptions{}) stores them, back to back.
    ``chunks`` (optional): the chunks' bytes themselves, in place of synthetic ones of
    ``sizes``."""

    def __init__(self, sizes, seed, chunks=None):
        if chunks is not None:
            sizes = [len(ch) for ch in chunks]
        self.sizes = [int(z) for z in sizes]
        self.offs = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.uint64)
        if chunks is None:
            self.plain = synthetic_bytes(self.offs, seed)
            self.chunks = [self.plain[int(a):int(b)].tobytes()
                           for a, b in zip(self.offs[:-1], self.offs[1:])]
        else:
            self.chunks = list(chunks)
            self.plain = np.frombuffer(b"".join(self.chunks), dtype=np.uint8).copy()
        n = len(self.sizes)
        self.refs = np.zeros(n, dtype=_lib.ref_dtype())
        self.hashes = np.zeros((n, 32), dtype=np.uint8)
        self.orefs, self.store, ctexts = [], {}, []
        for i, ch in enumerate(self.chunks):
            rid, dek, ct, h = created(ch)
            self.refs[i]["id"] = np.frombuffer(rid, dtype=np.uint8)
            self.refs[i]["dek"] = np.frombuffer(dek, dtype=np.uint8)
            self.hashes[i] = np.frombuffer(h, dtype=np.uint8)
            self.orefs.append(Ch.Ref(size_bytes=len(ch), edge=False, id=rid, dek=dek))
            self.store[rid] = ct
            ctexts.append(ct)
        self.ctext = np.frombuffer(b"".join(ctexts), dtype=np.uint8).copy()

    def oracle(self, slices) -> bytes:
        return b"".join(Ch.read_data_ref(self.store, Ch.DataRef(self.orefs[c], b"", o, z))
                        for c, o, z in slices)

    def sliced(self, slices) -> bytes:
        return b"".join(self.chunks[c][o:o + z] for c, o, z in slices)
