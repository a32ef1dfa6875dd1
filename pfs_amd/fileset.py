"""Host-side mirror of the reference's pachd write path above chunk.Writer, over the C ABI.

Reference interface (paths under /root/reference/src/internal/storage/fileset):

* ``Storage.NewUnorderedWriter(ctx, ...)``                         storage.go:84-92
* ``UnorderedWriter.Put(p, tag, appendFile, r) / Delete(p, tag) / Close()``
                                                                   unordered_writer.go:45-179
* ``fileset.Writer`` (Add / Delete / callback / Close) and the multilevel ``index.Writer``
  run inside the library per serialized fileset (writer.go:36-182, index/writer.go:27-162)
* ``Clean(p, isDir)``                                              util.go:67-77

Same names, argument meaning and error behaviour (errors are sticky; an out-of-order or
duplicate path inside a fileset is an error).  ``close()`` returns one ``Primitive`` per
serialized fileset (SizeBytes and the encoded root ``index.Index`` of the additive and
deletive indexes); the fileset ids and the composite of the Postgres metadata store, and the
chunk upload, are out of scope.  ``events`` records, per fileset, every formed chunk (data and
index streams, with its Ref.Id) and every level-0 index entry (pbutil frame).
"""
from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .cdc import ChunkParams, Chunker

DEFAULT_FILE_TAG = "default"
DEFAULT_MEMORY_THRESHOLD = 10 ** 9


@dataclass
class Primitive:
    additive: Optional[bytes]
    deletive: Optional[bytes]
    size_bytes: int
    num_files: int
    num_deletes: int


def clean(p: str, is_dir: bool) -> str:
    out = C.create_string_buffer(len(p.encode()) + 4)
    rc = _lib.load().pfscdc_path_clean(p.encode(), int(is_dir), out, len(out))
    if rc:
        raise _lib.PfsCdcError(rc, "path_clean")
    return out.value.decode()


def _tar_error(rc: int, what: str):
    if rc == _lib.PFSCDC_EUNSUPPORTED:
        return _lib.PfsCdcError(rc, f"{what}: the entry needs a PAX header (non-ASCII name, a "
                                    "name over 100 bytes that does not split, or a size above "
                                    "8 GiB - 1), which is written only with pax=True")
    return ValueError(f"{what}: empty name, or a directory entry with content")


def tar_header(path: str, size: int) -> bytes:
    """The 512-byte USTAR header Go's archive/tar writes for ``tarutil.NewHeader(path, size)``
    (tarutil/tar.go:35-40; pfscdc_tar_header).  PfsCdcError(PFSCDC_EUNSUPPORTED) for an entry
    that needs PAX records, ValueError for an empty name or a directory with a size."""
    p = path.encode() if isinstance(path, str) else bytes(path)
    if b"\0" in p or not 0 <= size < 1 << 64:
        raise ValueError(f"tar entry {path!r}: NUL in the name or a size outside uint64")
    out = (C.c_uint8 * 512)()
    rc = _lib.load().pfscdc_tar_header(p, size, out)
    if rc:
        raise _tar_error(rc, f"tar entry {path!r}")
    return bytes(out)


def _tar_format(pax: bool) -> int:
    return _lib.TAR_USTAR | _lib.TAR_PAX if pax else _lib.TAR_USTAR


def tar_head(path: str, size: int, pax: bool = True) -> bytes:
    """Every byte in front of an entry's content (pfscdc_tar_head): the 512 bytes of
    ``tar_header`` for an entry USTAR can hold; with ``pax``, for an entry it cannot hold, what
    archive/tar's FormatPAX writes: the extended header block, the ``path`` / ``size`` records
    padded to 512, and the main header block.  PfsCdcError(PFSCDC_EUNSUPPORTED) for an entry
    that needs PAX without ``pax``, and for a PAX entry whose name has an empty, "." or ".."
    component; ValueError for an empty name or a directory with a size."""
    p = path.encode() if isinstance(path, str) else bytes(path)
    if b"\0" in p or not 0 <= size < 1 << 64:
        raise ValueError(f"tar entry {path!r}: NUL in the name or a size outside uint64")
    lib, n = _lib.load(), C.c_uint64()
    rc = lib.pfscdc_tar_head(p, size, _tar_format(pax), None, 0, C.byref(n))
    if rc == 0:
        out = (C.c_uint8 * n.value)()
        rc = lib.pfscdc_tar_head(p, size, _tar_format(pax), out, n.value, C.byref(n))
    if rc == _lib.PFSCDC_EUNSUPPORTED and pax:
        raise _lib.PfsCdcError(rc, f"tar entry {path!r}: a PAX entry's name that is not clean "
                                   "(or longer than 65,535 bytes)")
    if rc:
        raise _tar_error(rc, f"tar entry {path!r}")
    return bytes(out)


def _tar_pieces(files):
    """(path, first, count) triples and the flat DataRef list of [(path, [DataRef])]."""
    triples, flat = [], []
    for path, drs in files:
        triples.append((path, len(flat), len(drs)))
        flat.extend(drs)
    return triples, flat


def tar_layout(files, pax: bool = False):
    """``(entry_offsets, total)`` of the stream getFileTar writes for ``files``, a list of
    (path, [DataRef]) (pfscdc_tar_layout_format): entry i is stream bytes [entry_offsets[i],
    entry_offsets[i + 1]), the 1,024-byte trailer begins at entry_offsets[len(files)]."""
    triples, flat = _tar_pieces(files)
    tf = _lib.tar_files(triples)
    sizes = (C.c_uint64 * max(1, len(files)))(
        *[sum(d.size_bytes for d in drs) for _, drs in files])
    offs = (C.c_uint64 * (len(files) + 1))()
    total = C.c_uint64()
    rc = _lib.load().pfscdc_tar_layout_format(tf, len(files), sizes, _tar_format(pax), offs,
                                              C.byref(total))
    if rc:
        for path, drs in files:  # name the first file that cannot be written
            tar_head(path, sum(d.size_bytes for d in drs), pax)
        raise ValueError("tar_layout: a directory entry with DataRefs")
    return list(offs), total.value


class TarStream:
    """The stream ``GetFileTAR`` sends for ``files`` (api_server.go:508-531, getFileTar
    :578-593, fileset.WriteTarEntry util.go:42-53), read from ``storage``'s chunk store in
    windows (pfscdc_store_read_tar): each window's distinct chunks are uploaded and verified
    once, only the window's content bytes are decrypted, and headers, padding and trailer are
    formed on the GPU.  ``storage``: a ``chunk.Storage`` with a store; ``files``: a list of
    (path, [DataRef]) in stream order.  Errors as ``chunk.Reader``'s: ValueError, KeyError (a
    chunk missing from the store), PfsCdcError (PFSCDC_ECORRUPT: a chunk failed verification,
    nothing written; PFSCDC_EUNSUPPORTED: an entry that needs a PAX header).  ``pax`` (None:
    the storage's): such an entry is written in PAX format, as archive/tar writes it, instead
    of being refused; every other entry, and a stream without one, is the same bytes."""

    def __init__(self, storage, files, pax: Optional[bool] = None):
        self.files = [(p, list(drs)) for p, drs in files]
        self.device = storage.device
        self._store = storage.store
        self._set_pax(storage, pax)
        self.entry_offsets, self._total = tar_layout(self.files, self.pax)
        self._c = None

    def _set_pax(self, storage, pax: Optional[bool]) -> None:
        self.pax = bool(getattr(storage, "pax", False) if pax is None else pax)

    def _format(self, c) -> None:
        """This stream's format on the context about to lay it out or read it."""
        rc = c.lib.pfscdc_set_tar_format(c.ctx, _tar_format(self.pax))
        if rc:
            raise _lib.PfsCdcError(rc, "pfscdc_set_tar_format")

    def size(self) -> int:
        return self._total

    def _window(self, begin: int, length: Optional[int]) -> int:
        if begin < 0 or begin > self._total or begin % 512:
            raise ValueError("begin must be a multiple of 512 inside the stream")
        n = self._total - begin if length is None else min(length, self._total - begin)
        if n < 0 or (begin + n < self._total and n % 512):
            raise ValueError("length must be a multiple of 512 unless the window reaches the "
                             "end of the stream")
        return n

    def _arrays(self):
        """The files and DataRefs as the C ABI takes them (built once, checked first)."""
        from .chunk import _full

        if self._store is None:
            raise ValueError("the storage has no chunk store to read from")
        if self._c is None:
            triples, flat = _tar_pieces(self.files)
            for i, dr in enumerate(flat):
                if dr.offset_bytes < 0 or dr.size_bytes < 0 or \
                        dr.offset_bytes + dr.size_bytes > dr.ref.size_bytes:
                    raise ValueError(f"DataRef {i} reaches past its chunk")
            arr = (_lib.FullDataRef * max(1, len(flat)))()
            for i, d in enumerate(flat):
                arr[i] = _full(d)
            self._c = (_lib.tar_files(triples), len(triples), arr, flat)
        return self._c

    def _read(self, ptr, cap: int, on_device: int, begin: int, n: int, chunker=None) -> int:
        tf, nfiles, arr, flat = self._arrays()
        c = chunker if chunker is not None else Chunker(ChunkParams(), self.device)
        try:
            nw = C.c_uint64()
            self._format(c)
            rc = c.lib.pfscdc_store_read_tar(c.ctx, self._store._s, tf, nfiles, arr,
                                             len(flat), begin, n, ptr, cap, on_device,
                                             C.byref(nw))
            msg = c.lib.pfscdc_last_error(c.ctx)
        finally:
            if chunker is None:
                c.close()
        if rc == _lib.PFSCDC_ENOTFOUND:
            for d in flat:
                self._store.get(d.ref.id)  # raises KeyError for the missing id
            raise KeyError("chunk not in the store")
        if rc:
            raise _lib.PfsCdcError(rc, f"TarStream: {msg.decode() if msg else ''}")
        return nw.value

    def read(self, begin: int = 0, length: Optional[int] = None) -> bytes:
        """Stream bytes [begin, begin + length) (None: to the end)."""
        n = self._window(begin, length)
        buf = (C.c_uint8 * max(1, n))()
        got = self._read(buf, n, 0, begin, n)
        return bytes(memoryview(buf)[:got])

    def read_into(self, tensor, begin: int = 0, length: Optional[int] = None) -> int:
        """The same window into a contiguous torch uint8 tensor (CUDA: the stream stays on the
        device); returns the number of bytes written.  Nothing is written on an error."""
        n = self._window(begin, length)
        if tensor.dtype.itemsize != 1 or not tensor.is_contiguous():
            raise ValueError("read_into needs a contiguous uint8 tensor")
        if tensor.numel() < n:
            raise ValueError("tensor smaller than the window")
        if tensor.is_cuda:
            import torch

            torch.cuda.current_stream(tensor.device).synchronize()  # earlier writes have landed
        return self._read(tensor.data_ptr() if tensor.numel() else None, tensor.numel(),
                          int(tensor.is_cuda), begin, n)

    def windows(self, nbytes: int):
        """Consecutive windows of ``nbytes`` (a multiple of 512) covering the stream, as
        grpcutil.WithStreamingBytesWriter sends it."""
        if nbytes <= 0 or nbytes % 512:
            raise ValueError("window size must be a positive multiple of 512")
        self._arrays()
        c = Chunker(ChunkParams(), self.device)  # one context for the whole stream
        try:
            buf = (C.c_uint8 * nbytes)()
            for begin in range(0, self._total, nbytes):
                got = self._read(buf, nbytes, 0, begin, self._window(begin, nbytes), c)
                yield bytes(memoryview(buf)[:got])
        finally:
            c.close()


@dataclass
class FileEntry:
    """One level-0 index entry: a file (or one tag of it) with its DataRefs."""
    path: str
    tag: str
    size_bytes: int
    data_refs: list


def _filter(lower, upper, prefix, tag):
    """pfscdc_index_filter of the four optional strings (None when all are unset)."""
    vals = [v.encode() if isinstance(v, str) else v for v in (lower, upper, prefix, tag)]
    if not any(vals):
        return None
    return _lib.IndexFilter(*[v or None for v in vals])


class IndexList:
    """An owned pfscdc_index_list: entries in stream order over one string blob and one
    pfscdc_full_dataref array."""

    def __init__(self, ptr):
        self.lib = _lib.load()
        self._p = ptr

    def __len__(self) -> int:
        return self.lib.pfscdc_index_list_count(self._p)

    def _views(self):
        n = len(self)
        ents = self.lib.pfscdc_index_list_entries(self._p)
        blen, ndr = C.c_uint64(), C.c_uint32()
        bp = self.lib.pfscdc_index_list_blob(self._p, C.byref(blen))
        blob = C.string_at(bp, blen.value) if blen.value else b""
        drs = self.lib.pfscdc_index_list_datarefs(self._p, C.byref(ndr))
        return n, ents, blob, drs, ndr.value

    @staticmethod
    def _dataref(d):
        from .chunk import DataRef, Ref
        return DataRef(Ref(d.ref_size, bool(d.edge), -1, bytes(d.ref.id), bytes(d.ref.dek)),
                       bytes(d.data.hash), d.data.offset_bytes, d.data.size_bytes)

    def raw(self) -> list:
        """Every entry as a dict of all its fields (paths and tags as bytes)."""
        n, ents, blob, drs, _ = self._views()
        out = []
        for i in range(n):
            e = ents[i]
            d = {"path": blob[e.path_off:e.path_off + e.path_len],
                 "tag": blob[e.tag_off:e.tag_off + e.tag_len],
                 "has_file": bool(e.flags & _lib.IDX_HAS_FILE),
                 "size_bytes": e.size_bytes,
                 "data_refs": [self._dataref(drs[k]) for k in range(e.first, e.first + e.count)],
                 "range": None}
            if e.flags & _lib.IDX_HAS_RANGE:
                ref = self._dataref(drs[e.first + e.count]) \
                    if e.flags & _lib.IDX_HAS_CHUNK_REF else None
                d["range"] = (e.range_offset,
                              blob[e.last_path_off:e.last_path_off + e.last_path_len], ref)
            out.append(d)
        return out

    def files(self) -> list:
        return [FileEntry(d["path"].decode("utf-8", "surrogateescape"),
                          d["tag"].decode("utf-8", "surrogateescape"), d["size_bytes"],
                          d["data_refs"]) for d in self.raw()]

    def free(self) -> None:
        if getattr(self, "_p", None):
            self.lib.pfscdc_index_list_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def index_decode_host(stream: bytes) -> IndexList:
    """pfscdc_index_decode_host: every entry of one level's stream of pbutil frames, decoded on
    the host.  PfsCdcError(PFSCDC_ECORRUPT) names the offset of the frame that does not parse."""
    out, err = C.c_void_p(), C.c_uint64()
    rc = _lib.load().pfscdc_index_decode_host(stream, len(stream), C.byref(out), C.byref(err))
    if rc:
        raise _lib.PfsCdcError(rc, f"index stream does not parse at offset {err.value}")
    return IndexList(out)


def index_filter(lst: IndexList, lower=None, upper=None, prefix=None, tag=None) -> IndexList:
    """Reader.Iterate's selection over a level-0 list (pfscdc_index_filter_list)."""
    f = _filter(lower, upper, prefix, tag)
    out = C.c_void_p()
    rc = _lib.load().pfscdc_index_filter_list(lst._p, C.byref(f) if f is not None else None,
                                              C.byref(out))
    if rc:
        raise _lib.PfsCdcError(rc, "pfscdc_index_filter_list")
    return IndexList(out)


def index_merge(pairs, chunker=None, deletive: bool = False) -> IndexList:
    """MergeReader.iterate over (deletive list, additive list) pairs in fileset order
    (pfscdc_index_merge); None stands for an empty list.  ``deletive``: iterateDeletive over
    the pairs' deletive lists (pfscdc_index_merge_deletive).  With a ``chunker`` the merge goes
    through pfscdc_index_merge_ctx on its context: on the device or on the host by the
    PFSCDC_INDEX_MERGE knob, with the same list either way."""
    pairs = list(pairs)
    lists = [d for d, _ in pairs] if deletive else [x for d, a in pairs for x in (d, a)]
    arr = (C.c_void_p * max(1, len(lists)))()
    for i, l in enumerate(lists):
        arr[i] = l._p if l is not None else None
    out = C.c_void_p()
    if chunker is not None:
        rc = chunker.lib.pfscdc_index_merge_ctx(
            chunker.ctx, _lib.MERGE_DELETIVE if deletive else _lib.MERGE_FILES, arr, len(pairs),
            C.byref(out))
        if rc:
            msg = chunker.lib.pfscdc_last_error(chunker.ctx)
            raise _lib.PfsCdcError(rc, f"index merge: {msg.decode() if msg else ''}")
        return IndexList(out)
    lib = _lib.load()
    fn = lib.pfscdc_index_merge_deletive if deletive else lib.pfscdc_index_merge
    rc = fn(arr, len(pairs), C.byref(out))
    if rc:
        raise _lib.PfsCdcError(rc, fn.__name__)
    return IndexList(out)


def last_merge_stats(chunker) -> dict:
    """Counts and stage times (ms) of the last index_merge on ``chunker``'s context."""
    n, ms = (C.c_uint64 * 4)(), (C.c_float * 4)()
    chunker.lib.pfscdc_last_merge_stats(chunker.ctx, n)
    chunker.lib.pfscdc_last_merge_timings(chunker.ctx, ms)
    out = dict(zip(["device", "entries_in", "groups", "entries_out"], [int(x) for x in n]))
    out.update(zip(["upload_ms", "rank_group_ms", "emit_ms", "d2h_ms"],
                   [round(float(x), 4) for x in ms]))
    return out


def shard(files: IndexList, threshold: int = DEFAULT_MEMORY_THRESHOLD) -> list:
    """shard (shard.go:27-49) over a merged list: the (lower, upper) path ranges, "" an open
    end (pfscdc_shard)."""
    out = []

    def cb(_user, lower, upper):
        out.append((lower.decode("utf-8", "surrogateescape"),
                    upper.decode("utf-8", "surrogateescape")))
        return 0

    rc = _lib.load().pfscdc_shard(files._p if files is not None else None, threshold,
                                  _lib.SHARD_CB(cb), None)
    if rc:
        raise _lib.PfsCdcError(rc, "pfscdc_shard")
    return out


def index_read(chunker, store, root: Optional[bytes], lower=None, upper=None, prefix=None,
               tag=None) -> IndexList:
    """index.NewReader(chunks, root, opts...).Iterate on ``chunker``'s context
    (pfscdc_index_read): the level-0 entries under ``root`` that the filter selects.  KeyError
    for a chunk missing from the store, PfsCdcError(PFSCDC_ECORRUPT) for a chunk that fails
    verification or a level that does not parse."""
    f = _filter(lower, upper, prefix, tag)
    out = C.c_void_p()
    rc = chunker.lib.pfscdc_index_read(chunker.ctx, store._s, root, len(root) if root else 0,
                                       C.byref(f) if f is not None else None, C.byref(out))
    if rc:
        msg = chunker.lib.pfscdc_last_error(chunker.ctx)
        msg = msg.decode() if msg else ""
        if rc == _lib.PFSCDC_ENOTFOUND:
            raise KeyError(msg or "chunk not in the store")
        raise _lib.PfsCdcError(rc, f"index read: {msg}")
    return IndexList(out)


def last_index_stats(chunker) -> dict:
    """Counts and stage times (ms) of the last index_read on ``chunker``'s context."""
    n, ms = (C.c_uint64 * 4)(), (C.c_float * 5)()
    chunker.lib.pfscdc_last_index_stats(chunker.ctx, n)
    chunker.lib.pfscdc_last_index_timings(chunker.ctx, ms)
    out = dict(zip(["chunks_read", "rewalked_chunks", "levels", "frames"], [int(x) for x in n]))
    out.update(zip(["verify_ms", "gather_ms", "walk_ms", "decode_ms", "d2h_ms"],
                   [round(float(x), 4) for x in ms]))
    return out


class DevIndexList:
    """An owned pfscdc_dev_list: the three arrays of an index list on the GPU (what the decode
    and merge kernels wrote, or an uploaded ``IndexList``); only the counts are on the host."""

    def __init__(self, ptr, device: int):
        self.lib = _lib.load()
        self._p = ptr
        self.device = device

    def __len__(self) -> int:
        return int(self.lib.pfscdc_dev_list_count(self._p))

    @property
    def num_datarefs(self) -> int:
        return int(self.lib.pfscdc_dev_list_num_datarefs(self._p))

    @property
    def blob_len(self) -> int:
        return int(self.lib.pfscdc_dev_list_blob_len(self._p))

    @classmethod
    def upload(cls, chunker, lst: Optional[IndexList]) -> "DevIndexList":
        out = C.c_void_p()
        rc = chunker.lib.pfscdc_dev_list_upload(chunker.ctx, lst._p if lst is not None else None,
                                                C.byref(out))
        if rc:
            raise _lib.PfsCdcError(rc, "pfscdc_dev_list_upload")
        return cls(out, chunker.device)

    def download(self, chunker=None) -> IndexList:
        """The list on the host, array for array."""
        c = chunker if chunker is not None else Chunker(ChunkParams(), self.device)
        try:
            out = C.c_void_p()
            rc = c.lib.pfscdc_dev_list_download(c.ctx, self._p, C.byref(out))
        finally:
            if chunker is None:
                c.close()
        if rc:
            raise _lib.PfsCdcError(rc, "pfscdc_dev_list_download")
        return IndexList(out)

    def free(self) -> None:
        if self._p:
            self.lib.pfscdc_dev_list_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def index_read_dev(chunker, store, root: Optional[bytes], lower=None, upper=None, prefix=None,
                   tag=None) -> DevIndexList:
    """``index_read`` with a resident result (pfscdc_index_read_dev): with no filter the level-0
    list stays on the device as the decode kernels wrote it."""
    f = _filter(lower, upper, prefix, tag)
    out = C.c_void_p()
    rc = chunker.lib.pfscdc_index_read_dev(chunker.ctx, store._s, root, len(root) if root else 0,
                                           C.byref(f) if f is not None else None, C.byref(out))
    if rc:
        msg = chunker.lib.pfscdc_last_error(chunker.ctx)
        msg = msg.decode() if msg else ""
        if rc == _lib.PFSCDC_ENOTFOUND:
            raise KeyError(msg or "chunk not in the store")
        raise _lib.PfsCdcError(rc, f"index read: {msg}")
    return DevIndexList(out, chunker.device)


def index_merge_dev(pairs, chunker, deletive: bool = False) -> DevIndexList:
    """``index_merge`` over resident (deletive, additive) pairs with a resident result
    (pfscdc_index_merge_dev); None stands for an empty list."""
    pairs = list(pairs)
    lists = [d for d, _ in pairs] if deletive else [x for d, a in pairs for x in (d, a)]
    arr = (C.c_void_p * max(1, len(lists)))()
    for i, l in enumerate(lists):
        arr[i] = l._p if l is not None else None
    out = C.c_void_p()
    rc = chunker.lib.pfscdc_index_merge_dev(
        chunker.ctx, _lib.MERGE_DELETIVE if deletive else _lib.MERGE_FILES, arr, len(pairs),
        C.byref(out))
    if rc:
        msg = chunker.lib.pfscdc_last_error(chunker.ctx)
        raise _lib.PfsCdcError(rc, f"index merge: {msg.decode() if msg else ''}")
    return DevIndexList(out, chunker.device)


def last_resident_stats(chunker) -> dict:
    """Counts of the last resident calls on ``chunker``'s context
    (pfscdc_last_resident_stats)."""
    n = (C.c_uint64 * 8)()
    chunker.lib.pfscdc_last_resident_stats(chunker.ctx, n)
    return dict(zip(["read_resident", "read_uploaded_bytes", "runs", "chunks", "pieces",
                     "d2h_bytes", "h2d_bytes", "plan_reused"], [int(x) for x in n]))


class _DevTarStream(TarStream):
    """TarStream over a resident list: layout and windows through pfscdc_dev_list_tar_layout
    and pfscdc_dev_list_read_tar; nothing per file or per DataRef comes to the host."""

    def __init__(self, storage, dev: DevIndexList, pax: Optional[bool] = None):
        self._dev = dev
        self.device = storage.device
        self._store = storage.store
        self._set_pax(storage, pax)
        self._offsets = None
        self.last_stats = None
        c = Chunker(ChunkParams(), self.device)
        try:
            total = C.c_uint64()
            self._format(c)
            rc = c.lib.pfscdc_dev_list_tar_layout(c.ctx, dev._p, C.byref(total), None)
            msg = c.lib.pfscdc_last_error(c.ctx)
        finally:
            c.close()
        if rc:
            raise _lib.PfsCdcError(rc, f"tar: {msg.decode('utf-8', 'replace') if msg else ''}")
        self._total = total.value

    @property
    def entry_offsets(self) -> list:
        if self._offsets is None:
            c = Chunker(ChunkParams(), self.device)
            try:
                offs, total = (C.c_uint64 * (len(self._dev) + 1))(), C.c_uint64()
                self._format(c)
                rc = c.lib.pfscdc_dev_list_tar_layout(c.ctx, self._dev._p, C.byref(total), offs)
            finally:
                c.close()
            if rc:
                raise _lib.PfsCdcError(rc, "pfscdc_dev_list_tar_layout")
            self._offsets = list(offs)
        return self._offsets

    def _arrays(self):
        if self._store is None:
            raise ValueError("the storage has no chunk store to read from")
        return None

    def _read(self, ptr, cap: int, on_device: int, begin: int, n: int, chunker=None) -> int:
        self._arrays()
        c = chunker if chunker is not None else Chunker(ChunkParams(), self.device)
        try:
            nw = C.c_uint64()
            self._format(c)
            rc = c.lib.pfscdc_dev_list_read_tar(c.ctx, self._store._s, self._dev._p, begin, n, ptr,
                                                cap, on_device, C.byref(nw))
            msg = c.lib.pfscdc_last_error(c.ctx)
            self.last_stats = last_resident_stats(c)
        finally:
            if chunker is None:
                c.close()
        if rc == _lib.PFSCDC_ENOTFOUND:
            raise KeyError("chunk not in the store")
        if rc:
            raise _lib.PfsCdcError(rc, f"TarStream: {msg.decode() if msg else ''}")
        return nw.value


FILE, DIR = _lib.FILE_TYPE_FILE, _lib.FILE_TYPE_DIR


@dataclass
class FileInfo:
    """``pfs.FileInfo`` as ``source.Iterate`` computes it: ``type`` is ``FILE`` or ``DIR`` (the
    path ends in '/'), ``size`` a file's bytes or the sum over a directory's subtree, ``hash``
    a file's ``hashDataRefs`` (or ``MergeFileReader.Hash``) or BLAKE2b-256 over a directory's
    immediate children's hashes."""
    path: str
    tag: str
    type: int
    size: int
    hash: bytes


def _leaf_ptr(leaf):
    if leaf is None:
        return None, None, 0
    if hasattr(leaf, "data_ptr"):  # a torch uint8 tensor
        return leaf.data_ptr() if leaf.numel() else None, leaf, int(leaf.is_cuda)
    buf = (C.c_uint8 * max(1, len(leaf))).from_buffer_copy(bytes(leaf) or b"\0")
    return C.cast(buf, C.c_void_p), buf, 0


def source_host(lst: Optional[IndexList], kind: int, arg: str = "", leaf=None):
    """pfscdc_source_host: the Source of a level-0 list on the host, ``(IndexList, infos)`` with
    one (hash, size, type, flags) per entry.  ``leaf``: 32 bytes per entry of ``lst`` used as
    the files' hashes.  KeyError where the reference answers file-not-found."""
    lib = _lib.load()
    out, infos = C.c_void_p(), C.POINTER(_lib.FileInfoC)()
    ptr, keep, _ = _leaf_ptr(leaf)
    rc = lib.pfscdc_source_host(lst._p if lst is not None else None, kind,
                                arg.encode("utf-8", "surrogateescape"), ptr, C.byref(out),
                                C.byref(infos))
    del keep
    if rc:
        msg = lib.pfscdc_source_host_error().decode("utf-8", "replace")
        if rc == _lib.PFSCDC_ENOTFOUND:
            raise KeyError(msg)
        raise _lib.PfsCdcError(rc, msg)
    res = IndexList(out)
    try:
        got = [(bytes(infos[i].hash), infos[i].size, infos[i].type, infos[i].flags)
               for i in range(len(res))]
    finally:
        lib.pfscdc_file_infos_free(infos)
    return res, got


GLOB_BYTES = "*?[]{}!()@+^\\"


def _glob_kind(p: str) -> int:
    """PFSCDC_SRC_GLOB if ``cleanPath(p)`` holds a glob byte, else PFSCDC_SRC_GET."""
    q = clean(p, False)
    return _lib.SRC_GLOB if any(c in q for c in GLOB_BYTES) else _lib.SRC_GET


def _glob_error(rc: int):
    return _lib.PfsCdcError(rc, _lib.load().pfscdc_source_host_error().decode("utf-8", "replace"))


def glob_match(glob: str, path: str) -> bool:
    """pfscdc_glob_match: ``globMatchFunction(cleanPath(glob))(path)``, the backtracking matcher
    that is the specification of the dialect (no GPU call).  PfsCdcError for a glob that does not
    compile (PFSCDC_EINVAL) or that holds extglob (PFSCDC_EUNSUPPORTED)."""
    hit = C.c_int(0)
    rc = _lib.load().pfscdc_glob_match(glob.encode("utf-8", "surrogateescape"),
                                       path.encode("utf-8", "surrogateescape"), C.byref(hit))
    if rc:
        raise _glob_error(rc)
    return bool(hit.value)


def glob_literal_prefix(glob: str) -> str:
    """pfscdc_glob_literal_prefix: ``globLiteralPrefix(cleanPath(glob))``."""
    out = C.create_string_buffer(len(glob.encode("utf-8", "surrogateescape")) + 8)
    rc = _lib.load().pfscdc_glob_literal_prefix(glob.encode("utf-8", "surrogateescape"), out,
                                                len(out))
    if rc:
        raise _lib.PfsCdcError(rc, "pfscdc_glob_literal_prefix")
    return out.value.decode("utf-8", "surrogateescape")


def glob_program(glob: str) -> dict:
    """pfscdc_debug_glob_program (a test hook): the position automaton of ``cleanPath(glob)``
    as the device stages it: ``follow`` (64) and ``accept_byte`` (256) as uint64 arrays,
    ``first``, ``last``, ``nullable`` and ``positions``."""
    out = (C.c_uint64 * 324)()
    rc = _lib.load().pfscdc_debug_glob_program(glob.encode("utf-8", "surrogateescape"), out)
    if rc:
        raise _glob_error(rc)
    w = np.frombuffer(out, dtype=np.uint64).copy()
    return {"follow": w[:64], "accept_byte": w[64:320], "first": int(w[320]), "last": int(w[321]),
            "nullable": bool(w[322]), "positions": int(w[323])}


def glob_masks(chunker, lst: "DevIndexList", glob: str):
    """pfscdc_debug_glob_masks (a test hook): the glob kernel alone over a resident list;
    ``(masks, bad)`` with one uint64 per entry."""
    n = len(lst)
    masks = np.zeros(max(1, n), dtype=np.uint64)
    bad = C.c_uint32(0)
    rc = chunker.lib.pfscdc_debug_glob_masks(
        chunker.ctx, lst._p, glob.encode("utf-8", "surrogateescape"),
        masks.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(bad))
    if rc:
        msg = chunker.lib.pfscdc_last_error(chunker.ctx)
        raise _lib.PfsCdcError(rc, msg.decode("utf-8", "replace") if msg else "")
    return masks[:n], int(bad.value)


_LIST_SCAN_KINDS = (  # pfscdc_debug_list_scan: a record's dtype and its columns
    (np.dtype([("ndr", "<u4"), ("blob", "<u4")]), 2),
    (np.dtype([("emit", "<u4"), ("recs", "<u4"), ("blob", "<u8")]), 3),
    (np.dtype("<u8"), 1),
)


def list_scan(chunker, kind: int, records):
    """pfscdc_debug_list_scan (a test hook): kind's prefix-sum kernel of the list passes alone over
    ``records`` (``_LIST_SCAN_KINDS[kind]``'s dtype); a uint64 array of shape (n + 1, columns),
    row i the sums before record i, the last row the totals."""
    dtype, cols = _LIST_SCAN_KINDS[kind]
    rec = np.ascontiguousarray(records, dtype=dtype)
    out = np.zeros((len(rec) + 1, cols), dtype=np.uint64)
    rc = chunker.lib.pfscdc_debug_list_scan(
        chunker.ctx, kind, rec.ctypes.data_as(C.c_void_p), len(rec),
        out.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc:
        msg = chunker.lib.pfscdc_last_error(chunker.ctx)
        raise _lib.PfsCdcError(rc, msg.decode("utf-8", "replace") if msg else "")
    return out


class _BorrowedDevList(DevIndexList):
    """A source's list: owned by the source, which it keeps alive."""

    def __init__(self, ptr, device, owner):
        super().__init__(ptr, device)
        self._owner = owner

    def free(self) -> None:
        self._p = None
        self._owner = None


class Source:
    """An owned pfscdc_source: the selected entries with their directories as a resident list
    (``list``: what the tar calls take) and one FileInfo record per entry on the GPU."""

    def __init__(self, ptr, device: int):
        self.lib = _lib.load()
        self._p = ptr
        self.device = device

    def __len__(self) -> int:
        return int(self.lib.pfscdc_source_count(self._p))

    @property
    def list(self) -> DevIndexList:
        return _BorrowedDevList(self.lib.pfscdc_source_list(self._p), self.device, self)

    def infos(self, chunker=None) -> list:
        """(hash, size, type, flags) per entry."""
        c = chunker if chunker is not None else Chunker(ChunkParams(), self.device)
        try:
            n = len(self)
            arr = (_lib.FileInfoC * max(1, n))()
            rc = c.lib.pfscdc_source_infos(c.ctx, self._p, arr)
        finally:
            if chunker is None:
                c.close()
        if rc:
            raise _lib.PfsCdcError(rc, "pfscdc_source_infos")
        return [(bytes(arr[i].hash), arr[i].size, arr[i].type, arr[i].flags) for i in range(n)]

    def free(self) -> None:
        if self._p:
            self.lib.pfscdc_source_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def source_open(chunker, lst, kind: int, arg: str = "", leaf=None) -> Source:
    """pfscdc_source_open over a ``DevIndexList`` (pfscdc_source_open_list over an ``IndexList``
    or None, uploaded first): on the device or on the host by the PFSCDC_SOURCE knob, with the
    same result either way.  ``leaf``: bytes or a torch uint8 tensor (host or device), 32 bytes
    per entry of ``lst``.  KeyError where the reference answers file-not-found."""
    out = C.c_void_p()
    ptr, keep, on_dev = _leaf_ptr(leaf)
    fn = chunker.lib.pfscdc_source_open if isinstance(lst, DevIndexList) \
        else chunker.lib.pfscdc_source_open_list
    rc = fn(chunker.ctx, lst._p if lst is not None else None, kind,
            arg.encode("utf-8", "surrogateescape"), ptr, on_dev, C.byref(out))
    del keep
    if rc:
        msg = chunker.lib.pfscdc_last_error(chunker.ctx)
        msg = msg.decode("utf-8", "replace") if msg else ""
        if rc == _lib.PFSCDC_ENOTFOUND:
            raise KeyError(msg)
        raise _lib.PfsCdcError(rc, msg)
    return Source(out, chunker.device)


def last_source_stats(chunker) -> dict:
    """Counts and stage times (ms) of the last source_open on ``chunker``'s context."""
    n, ms = (C.c_uint64 * 8)(), (C.c_float * 4)()
    chunker.lib.pfscdc_last_source_stats(chunker.ctx, n)
    chunker.lib.pfscdc_last_source_timings(chunker.ctx, ms)
    out = dict(zip(["device", "entries_in", "entries_out", "dirs_inserted", "levels",
                    "hash_launches", "h2d_bytes", "d2h_bytes"], [int(x) for x in n]))
    out.update(zip(["select_ms", "tree_ms", "leaf_ms", "levels_ms"],
                   [round(float(x), 4) for x in ms]))
    return out


def _infos_array(infos):
    arr = (_lib.FileInfoC * max(1, len(infos)))()
    for i, (h, size, typ, flags) in enumerate(infos):
        arr[i] = _lib.FileInfoC((C.c_uint8 * 32)(*h), size, typ, flags)
    return arr


def diff_host(a: Optional[IndexList], a_infos, b: Optional[IndexList], b_infos) -> list:
    """pfscdc_diff_host: ``Differ.Iterate``'s two-pointer walk over two sides on the host, each a
    list with its (hash, size, type, flags) per entry as ``source_host`` returns them (None: an
    empty side).  One ``(i, j)`` per callback, in callback order: indexes into the sides, None
    for the side the callback got nil for."""
    lib = _lib.load()
    out, n = C.POINTER(_lib.DiffPairC)(), C.c_uint64()
    rc = lib.pfscdc_diff_host(a._p if a is not None else None, _infos_array(a_infos or []),
                              b._p if b is not None else None, _infos_array(b_infos or []),
                              C.byref(out), C.byref(n))
    if rc:
        raise _lib.PfsCdcError(rc, "pfscdc_diff_host")
    try:
        return [(None if out[k].a == _lib.DIFF_NONE else out[k].a,
                 None if out[k].b == _lib.DIFF_NONE else out[k].b) for k in range(n.value)]
    finally:
        lib.pfscdc_diff_pairs_free(out)


class _BorrowedSource(Source):
    """A diff's selection: owned by the diff, which it keeps alive."""

    def __init__(self, ptr, device, owner):
        super().__init__(ptr, device)
        self._owner = owner

    def free(self) -> None:
        self._p = None
        self._owner = None


class Diff:
    """An owned pfscdc_diff: the pairs ``Differ.Iterate`` reports, and per side the entries that
    occur in them as a ``Source`` of their own (``side(0)``: the old commit's, ``side(1)``: the
    new one's), all on the GPU."""

    def __init__(self, ptr, device: int):
        self.lib = _lib.load()
        self._p = ptr
        self.device = device

    def __len__(self) -> int:
        return int(self.lib.pfscdc_diff_count(self._p))

    def pairs(self, chunker) -> list:
        """``(i, j)`` per pair as ``diff_host`` gives them."""
        n = len(self)
        arr = (_lib.DiffPairC * max(1, n))()
        rc = chunker.lib.pfscdc_diff_pairs(chunker.ctx, self._p, arr)
        if rc:
            raise _lib.PfsCdcError(rc, "pfscdc_diff_pairs")
        return [(None if arr[k].a == _lib.DIFF_NONE else arr[k].a,
                 None if arr[k].b == _lib.DIFF_NONE else arr[k].b) for k in range(n)]

    def side(self, which: int) -> Source:
        p = self.lib.pfscdc_diff_side(self._p, which)
        if not p:
            raise ValueError("a diff has sides 0 and 1")
        return _BorrowedSource(p, self.device, self)

    def free(self) -> None:
        if self._p:
            self.lib.pfscdc_diff_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def source_diff(chunker, a: Optional[Source], b: Source) -> Diff:
    """pfscdc_source_diff: the walk over two Sources of ``chunker``'s device (``a`` None: the nil
    parent commit), on the device or on the host by the PFSCDC_DIFF knob, with the same result
    either way."""
    out = C.c_void_p()
    rc = chunker.lib.pfscdc_source_diff(chunker.ctx, a._p if a is not None else None,
                                        b._p if b is not None else None, C.byref(out))
    if rc:
        msg = chunker.lib.pfscdc_last_error(chunker.ctx)
        raise _lib.PfsCdcError(rc, msg.decode("utf-8", "replace") if msg else "")
    return Diff(out, chunker.device)


def last_diff_stats(chunker) -> dict:
    """Counts and stage times (ms) of the last source_diff on ``chunker``'s context."""
    n, ms = (C.c_uint64 * 8)(), (C.c_float * 4)()
    chunker.lib.pfscdc_last_diff_stats(chunker.ctx, n)
    chunker.lib.pfscdc_last_diff_timings(chunker.ctx, ms)
    out = dict(zip(["device", "entries_a", "entries_b", "pairs", "both", "h2d_bytes",
                    "d2h_bytes"], [int(x) for x in n]))
    out.update(zip(["rank_ms", "fill_ms", "select_ms", "guards_ms"],
                   [round(float(x), 4) for x in ms]))
    return out


def _path_arg(p: str) -> bytes:
    return p.encode("utf-8", "surrogateescape")


def copy_map_host(lst: Optional[IndexList], src: str, dst: str, src_tag: str = "") -> IndexList:
    """pfscdc_copy_map_host: CopyFile's selection and path transform of a level-0 list on the
    host: the entries ``copyFile`` selects for ``src`` (and ``src_tag``, "" for every tag) with
    their paths moved under ``dst``."""
    lib = _lib.load()
    out = C.c_void_p()
    rc = lib.pfscdc_copy_map_host(lst._p if lst is not None else None, _path_arg(src),
                                  _path_arg(src_tag), _path_arg(dst), C.byref(out))
    if rc:
        raise _lib.PfsCdcError(rc, "pfscdc_copy_map_host")
    return IndexList(out)


def copy_map(chunker, lst_or_dev, src: str, dst: str, src_tag: str = "") -> DevIndexList:
    """pfscdc_dev_list_copy_map over a ``DevIndexList`` (pfscdc_copy_map_list over an
    ``IndexList`` or None, uploaded first): on the device or on the host by the PFSCDC_COPY_MAP
    knob, with the same result either way."""
    out = C.c_void_p()
    fn = chunker.lib.pfscdc_dev_list_copy_map if isinstance(lst_or_dev, DevIndexList) \
        else chunker.lib.pfscdc_copy_map_list
    rc = fn(chunker.ctx, lst_or_dev._p if lst_or_dev is not None else None, _path_arg(src),
            _path_arg(src_tag), _path_arg(dst), C.byref(out))
    if rc:
        msg = chunker.lib.pfscdc_last_error(chunker.ctx)
        raise _lib.PfsCdcError(rc, msg.decode("utf-8", "replace") if msg else "copy map")
    return DevIndexList(out, chunker.device)


def last_copy_map_stats(chunker) -> dict:
    """Counts and stage times (ms) of the last copy_map on ``chunker``'s context."""
    n, ms = (C.c_uint64 * 8)(), (C.c_float * 4)()
    chunker.lib.pfscdc_last_copy_map_stats(chunker.ctx, n)
    chunker.lib.pfscdc_last_copy_map_timings(chunker.ctx, ms)
    out = dict(zip(["device", "entries_in", "entries_out", "datarefs_out", "blob_bytes_out",
                    "h2d_bytes", "d2h_bytes"], [int(x) for x in n]))
    out.update(zip(["count_ms", "fill_ms", "copy_ms", "guards_ms"],
                   [round(float(x), 4) for x in ms]))
    return out


class _SourceTarStream(_DevTarStream):
    """GetFileTAR as the reference serves it: one tar entry per entry of a source's stream,
    directories included."""

    def __init__(self, storage, source: Source, pax: Optional[bool] = None):
        self._source = source
        super().__init__(storage, source.list, pax)


class _FlatRefs:
    """The DataRefs of an IndexList as TarStream looks at them: their count, and their Ref
    ids when a missing chunk has to be named."""

    def __init__(self, lst: IndexList):
        self._l = lst

    def __len__(self) -> int:
        return self._l._views()[4]

    def __iter__(self):
        _, _, _, drs, n = self._l._views()
        return (IndexList._dataref(drs[k]) for k in range(n))


class _ListTarStream(TarStream):
    """TarStream over a merged IndexList: the list's own pfscdc_tar_file and
    pfscdc_full_dataref arrays go to pfscdc_store_read_tar as they are."""

    def __init__(self, storage, lst: IndexList, pax: Optional[bool] = None):
        self._list = lst
        self.device = storage.device
        self._store = storage.store
        self._set_pax(storage, pax)
        n, ents, blob, drs, ndr = lst._views()
        lib = lst.lib
        self._tf = lib.pfscdc_index_list_tar_files(lst._p)
        sizes = (C.c_uint64 * max(1, n))(*[ents[i].size_bytes for i in range(n)])
        offs, total = (C.c_uint64 * (n + 1))(), C.c_uint64()
        rc = lib.pfscdc_tar_layout_format(self._tf, n, sizes, _tar_format(self.pax), offs,
                                          C.byref(total))
        if rc:
            for i in range(n):  # name the first file that cannot be written
                e = ents[i]
                tar_head(blob[e.path_off:e.path_off + e.path_len].decode("utf-8", "replace"),
                         e.size_bytes, self.pax)
            raise ValueError("tar: a directory entry with DataRefs")
        self.entry_offsets, self._total = list(offs), total.value
        self._c = (self._tf, n, drs, _FlatRefs(lst))

    def _arrays(self):
        if self._store is None:
            raise ValueError("the storage has no chunk store to read from")
        return self._c


class FileSet:
    """The merged view of opened filesets (``Storage.open``): the files that
    ``MergeReader.iterate`` yields, in path-then-tag order."""

    def __init__(self, storage, merged: Optional[IndexList], resident: Optional[DevIndexList] = None,
                 nfilesets: int = 1):
        self._storage, self._host, self._dev = storage, merged, resident
        self._nfilesets = nfilesets
        self._leaf = None  # MergeFileReader.Hash per file, made on first use

    @property
    def _list(self) -> IndexList:
        """The merged list on the host (a resident fileset downloads it once, on first use)."""
        if self._host is None:
            self._host = self._dev.download()
        return self._host

    @property
    def resident(self) -> Optional[DevIndexList]:
        """The merged list on the device (``Storage.open(..., resident=True)``), else None."""
        return self._dev

    def files(self) -> list:
        """``FileEntry`` (path, tag, size, DataRefs) per merged file."""
        return self._list.files()

    def read(self, path: str) -> bytes:
        """The content of ``path``: its entries' DataRefs in tag order, through the chunk
        read path (pfscdc_store_read).  KeyError if the fileset has no such file."""
        from .chunk import Storage as ChunkStorage
        drs = [d for f in self.files() if f.path == path for d in f.data_refs]
        if not any(f.path == path for f in self.files()):
            raise KeyError(path)
        return ChunkStorage(self._storage.device, store=self._storage.store).new_reader(drs).get()

    def tar(self, pax: Optional[bool] = None) -> TarStream:
        """``GetFileTAR`` over the merged files (a ``TarStream``; ``pax`` as ``TarStream``'s)."""
        if self._dev is not None:
            return _DevTarStream(self._storage, self._dev, pax)
        return _ListTarStream(self._storage, self._list, pax)

    # ---- the file RPCs over a Source (driver_file.go:173-385)

    def _source(self, kind: int, arg: str) -> Source:
        """The opened filesets wrapped in a Source.  A resident fileset feeds its list straight
        in, a host one uploads; opened over more than one fileset the files' hashes are
        ``MergeFileReader.Hash`` (storage.go:124-127), else ``hashDataRefs`` on the device."""
        if self._nfilesets > 1 and self._leaf is None:
            from .chunk import merge_file_hash
            self._leaf = b"".join(
                bytes(32) if f.path.endswith("/") else
                merge_file_hash(self._storage.store, f.data_refs, self._storage.device)
                for f in self.files())
        leaf = self._leaf
        c = Chunker(ChunkParams(), self._storage.device)
        try:
            return source_open(c, self._dev if self._dev is not None else self._host, kind, arg,
                               leaf)
        finally:
            c.close()

    def _infos(self, kind: int, arg: str, only: int = 0) -> list:
        """The source's FileInfos; ``only``: those with this PFSCDC_INFO_* flag."""
        src = self._source(kind, arg)
        try:
            raw, infos = src.list.download().raw(), src.infos()
        finally:
            src.free()
        return [FileInfo(d["path"].decode("utf-8", "surrogateescape"),
                         d["tag"].decode("utf-8", "surrogateescape"), t, size, h)
                for d, (h, size, t, flags) in zip(raw, infos)
                if not only or flags & only]

    def walk_file(self, p: str = "") -> list:
        """``walkFile``: the ``FileInfo`` of ``p`` and of everything below it, directories
        included ("" or "/": the whole commit; an empty commit gives []).  KeyError if nothing
        is there."""
        return self._infos(_lib.SRC_SUBTREE, p)

    def list_file(self, p: str = "") -> list:
        """``listFile``: the ``FileInfo`` of the immediate children of directory ``p`` (of the
        file ``p`` itself, if it is one)."""
        return self._infos(_lib.SRC_LIST, p, only=_lib.INFO_CHILD)

    def inspect_file(self, p: str = "") -> Optional[FileInfo]:
        """``inspectFile``: the ``FileInfo`` of ``p`` (the last entry with path ``p`` or
        ``p + "/"``).  KeyError if nothing is there."""
        q = clean(p, False)
        q = "" if q == "/" else q
        hits = [fi for fi in self._infos(_lib.SRC_SUBTREE, p) if fi.path in (q, q + "/")]
        return hits[-1] if hits else None

    def get_file(self, p: str, pax: Optional[bool] = None) -> TarStream:
        """``getFile`` as ``GetFileTAR`` serves it: what the glob ``p`` matches (each a file, or
        a directory with everything below it) as a ``TarStream`` with one entry per entry of the
        source, directories included.  A ``p`` with none of the glob bytes names one path.
        KeyError if nothing is there.  ``pax`` (None: the storage's): an entry USTAR cannot
        hold is written in PAX format instead of PfsCdcError(PFSCDC_EUNSUPPORTED)."""
        return _SourceTarStream(self._storage, self._source(_glob_kind(p), p), pax)

    def glob_file(self, pattern: str) -> list:
        """``globFile``: the ``FileInfo`` of every path the glob ``pattern`` matches itself; a
        matched directory's size and hash cover everything below it.  Nothing matched is []."""
        try:
            return self._infos(_lib.SRC_GLOB, pattern, only=_lib.INFO_MATCH)
        except KeyError:  # getFile's NewErrOnEmpty, which globFile does not wrap its stream in
            return []

    def diff_file(self, old: Optional["FileSet"], path: str = "",
                  old_path: Optional[str] = None) -> list:
        """``diffFile``: what differs between ``old_path`` (default: ``path``) in the commit
        ``old`` (None: the nil parent commit, an empty side) and ``path`` in this one, as
        ``(old FileInfo or None, new FileInfo or None)`` per callback of ``Differ.Iterate``,
        directories included.  A path one commit lacks is an empty side, not an error.  Both
        Sources and the join stay on the GPU; only the pairs and the entries that occur in them
        are downloaded."""
        new_src = self._source(_lib.SRC_DIFF, path)
        old_src = None
        c = Chunker(ChunkParams(), self._storage.device)
        try:
            if old is not None:
                old_src = old._source(_lib.SRC_DIFF, path if old_path is None else old_path)
            d = source_diff(c, old_src, new_src)
            try:
                pairs = d.pairs(c)
                sides = []
                for which in (0, 1):
                    s = d.side(which)
                    sides.append([FileInfo(r["path"].decode("utf-8", "surrogateescape"),
                                           r["tag"].decode("utf-8", "surrogateescape"), t, size, h)
                                  for r, (h, size, t, _) in zip(s.list.download(c).raw(), s.infos(c))])
            finally:
                d.free()
        finally:
            c.close()
            new_src.free()
            if old_src is not None:
                old_src.free()
        its = [iter(sides[0]), iter(sides[1])]
        return [(next(its[0]) if i is not None else None, next(its[1]) if j is not None else None)
                for i, j in pairs]


class Storage:
    """``fileset.Storage`` restricted to the write path and to reading filesets back, bound to
    one GPU, or with ``devices`` to a device group (one process, several GPUs:
    pfscdc_uw_create_group deals the serialized filesets over them; the filesets and events
    equal one GPU's).  ``store``: the chunk client; with one, every chunk the unordered writers
    form (data and index) is uploaded into it and ``open`` reads filesets back from it.
    ``pax``: the tar format of every ``TarStream`` opened from it (``FileSet.tar`` /
    ``get_file``), unless the call says otherwise: False refuses an entry USTAR cannot hold,
    True writes it in PAX format."""

    def __init__(self, device: int = 0, params: ChunkParams = ChunkParams(),
                 mem_threshold: int = DEFAULT_MEMORY_THRESHOLD,
                 index_params: Optional[ChunkParams] = None,
                 devices: Optional[Sequence[int]] = None, store=None, pax: bool = False):
        self.device, self.params = device, params
        self.pax = pax  # the tar format of everything opened from this storage (TarStream)
        self.devices = list(devices) if devices is not None else None
        self.mem_threshold, self.index_params = mem_threshold, index_params
        self.store = store
        self._idle: list = []  # data-stream contexts (or groups) of closed writers, for the next

    def new_unordered_writer(self) -> "UnorderedWriter":
        return UnorderedWriter(self)

    def open(self, filesets, lower=None, upper=None, prefix=None, tag=None,
             resident: bool = False) -> FileSet:
        """The merged view of ``filesets`` (the ``Primitive`` infos ``UnorderedWriter.close()``
        returns, (additive root, deletive root) pairs, or bare additive roots), in order:
        both indexes of every fileset are read with the filter (index.Reader over the store)
        and merged (MergeReader.iterate).  ``resident``: the lists stay on the GPU from the
        index read through the merge (pfscdc_index_read_dev, pfscdc_index_merge_dev) and
        ``tar()`` renders from there; ``files()`` and ``read()`` download the merged list on
        first use."""
        if self.store is None:
            raise ValueError("the storage has no chunk store to read from")
        roots = []
        for fs in filesets:
            if isinstance(fs, (bytes, bytearray)) or fs is None:
                roots.append((fs, None))
            elif isinstance(fs, tuple):
                roots.append(fs)
            else:
                roots.append((fs.additive, fs.deletive))
        c = Chunker(ChunkParams(), self.device)
        if resident:
            try:
                pairs = [(index_read_dev(c, self.store, d, lower, upper, prefix, tag),
                          index_read_dev(c, self.store, a, lower, upper, prefix, tag))
                         for a, d in roots]
                merged = index_merge_dev(pairs, c)
                for d, a in pairs:
                    d.free()
                    a.free()
            finally:
                c.close()
            return FileSet(self, None, merged, nfilesets=len(roots))
        try:
            pairs = [(index_read(c, self.store, d, lower, upper, prefix, tag),
                      index_read(c, self.store, a, lower, upper, prefix, tag))
                     for a, d in roots]
            merged = index_merge(pairs, chunker=c)
        finally:
            c.close()
        return FileSet(self, merged, nfilesets=len(roots))

    def shard(self, filesets, threshold: int = 10 ** 9) -> list:
        """``Storage.Shard`` (shard.go:12-18): the (lower, upper) path ranges, "" an open end,
        that split the merged view of ``filesets`` into runs of ``threshold`` content bytes."""
        return shard(self.open(filesets)._list, threshold)

    @staticmethod
    def _infos(filesets):
        """pfscdc_fileset_info array of ``Primitive``s, (additive, deletive) pairs or bare
        additive roots; the second value keeps the roots' buffers alive."""
        arr = (_lib.FilesetInfo * max(1, len(filesets)))()
        keep = []
        for i, fs in enumerate(filesets):
            if isinstance(fs, (bytes, bytearray)) or fs is None:
                a, d = fs, None
            elif isinstance(fs, tuple):
                a, d = fs
            else:
                a, d = fs.additive, fs.deletive
            for name, root in (("additive", a), ("deletive", d)):
                if root:
                    buf = C.create_string_buffer(bytes(root), len(root))
                    keep.append(buf)
                    setattr(arr[i], name + "_root", C.cast(buf, C.c_void_p))
                    setattr(arr[i], name + "_root_len", len(root))
        return arr, keep

    def new_writer(self) -> "FilesetWriter":
        """``Storage.newWriter``: a ``fileset.Writer`` with Delete and Copy."""
        return FilesetWriter(self)

    def compact(self, filesets, lower=None, upper=None, prefix=None) -> Primitive:
        """``Storage.Compact`` (compaction.go:43-57): ``filesets`` opened with the path range,
        merged, and copied into one new fileset (``CopyFiles(ctx, w, fs, true)``)."""
        w = self.new_writer()
        try:
            w.copy_filesets(filesets, lower, upper, prefix)
            return w.close()
        finally:
            w.release()

    def concat(self, filesets) -> Primitive:
        """``Storage.Concat`` (storage.go:226-238): each fileset copied in turn into one new
        fileset; their path ranges must not overlap and must come in order."""
        w = self.new_writer()
        try:
            for fs in filesets:
                w.copy_filesets([fs])
            return w.close()
        finally:
            w.release()

    def _take_chunker(self):
        # a context (stream, events, device staging) per GPU, reused writer after writer, as
        # a pachd process would hold it; a writer still open gets a context of its own
        if self._idle:
            return self._idle.pop()
        if self.devices is not None:
            from .group import DeviceGroup
            return DeviceGroup(self.devices, self.params, ref_ids=True)
        return Chunker(self.params, self.device, ref_ids=True)

    def _give_chunker(self, c) -> None:
        if getattr(c, "ctx", None) or getattr(c, "g", None):  # (not closed by a finalizer)
            self._idle.append(c)

    def trim(self) -> dict:
        """Free what closed writers left for the next one: this Storage's idle data contexts
        (stream, events, grow-only device staging) and, process-wide for this device, the
        pooled page-locked fileset arenas with their device mirrors and the cached index
        contexts (pfscdc_uw_trim_cache).  Call it with no writer open on this device."""
        lib = _lib.load()
        n_idle = len(self._idle)
        while self._idle:
            self._idle.pop().close()
        freed, ctxs = C.c_uint64(0), C.c_uint32(0)
        rc = lib.pfscdc_uw_trim_cache(self.device, C.byref(freed), C.byref(ctxs))
        if rc != 0:
            raise _lib.PfsCdcError(rc, "pfscdc_uw_trim_cache")
        return {"data_contexts": n_idle, "arena_bytes": int(freed.value),
                "cached_contexts": int(ctxs.value)}


class FilesetWriter:
    """``fileset.Writer`` over pfscdc_fsw_*: ``delete`` and ``copy`` in path order, ``close``
    returns the ``Primitive``.  ``events``: every formed chunk as ("chunk", index, level, size,
    edge, Ref.Id, copied) -- copied: a data chunk passed through by reference -- and every
    level-0 index entry as ("index", which, frame).  Errors are sticky."""

    def __init__(self, storage: Storage):
        self.lib = _lib.load()
        if storage.store is None:
            raise ValueError("the storage has no chunk store to copy from")
        self._storage = storage
        # one fileset on one GPU: a device group's Storage writes it on its first device
        self._own = storage.devices is not None
        self._chunker = Chunker(storage.params, storage.devices[0], ref_ids=True) if self._own \
            else storage._take_chunker()
        self.events: list = []
        self._exc: Optional[BaseException] = None
        ref = weakref.ref(self)

        def on_event(user, ev_p, _ref=ref):
            o = _ref()
            return o._on_event(user, ev_p) if o is not None else 1

        self._cfun = _lib.UW_CB(on_event)
        ip = storage.index_params.to_c() if storage.index_params else None
        w = C.c_void_p()
        rc = self.lib.pfscdc_fsw_create(self._chunker.ctx, C.byref(ip) if ip is not None else None,
                                        storage.store._s, self._cfun, None, C.byref(w))
        if rc:
            self.release()
            raise _lib.PfsCdcError(rc, "pfscdc_fsw_create")
        self._w = w

    def _on_event(self, _user, ev_p) -> int:
        try:
            ev = ev_p.contents
            if ev.kind == _lib.EV_CHUNK:
                ch = ev.chunk
                self.events.append(("chunk", ev.index, ev.level if ev.index >= 0 else 0,
                                    ch.size_bytes, bool(ch.edge), bytes(ch.ref.id),
                                    bool(ch.copied)))
            else:
                self.events.append(("index", ev.index, C.string_at(ev.bytes, ev.len)))
            return 0
        except BaseException as e:
            self._exc = e
            return 1

    def _check(self, rc: int, what: str) -> None:
        if self._exc is not None:
            exc, self._exc = self._exc, None
            raise exc
        if rc:
            msg = self.lib.pfscdc_fsw_last_error(self._w) if getattr(self, "_w", None) else None
            raise _lib.PfsCdcError(rc, f"{what}: {msg.decode() if msg else ''}")

    def delete(self, p: str, tag: str = "") -> None:
        self._check(self.lib.pfscdc_fsw_delete(self._w, p.encode(), tag.encode()), "Delete")

    def copy(self, p: str, tag: str, data_refs) -> None:
        """``Writer.Copy``: the file ``p`` under ``tag`` made of ``data_refs`` (DataRefs with
        their chunks' Refs, in the store)."""
        from .chunk import _full

        arr = (_lib.FullDataRef * max(1, len(data_refs)))()
        for i, d in enumerate(data_refs):
            arr[i] = _full(d)
        self._check(self.lib.pfscdc_fsw_copy(self._w, p.encode(), tag.encode(), arr,
                                             len(data_refs)), "Copy")

    def copy_lists(self, additive: Optional[IndexList], deletive: Optional[IndexList]) -> None:
        """``CopyFiles(ctx, w, fs, true)`` over an opened fileset's two lists."""
        self._check(self.lib.pfscdc_fsw_copy_lists(
            self._w, additive._p if additive is not None else None,
            deletive._p if deletive is not None else None), "CopyFiles")

    def copy_filesets(self, filesets, lower=None, upper=None, prefix=None) -> None:
        """``Open(ids, opts...)`` and ``CopyFiles``: the filesets read with the path range,
        merged and copied."""
        filesets = list(filesets)
        arr, keep = Storage._infos(filesets)
        f = _filter(lower, upper, prefix, None)
        self._check(self.lib.pfscdc_fsw_copy_filesets(
            self._w, arr, len(filesets), C.byref(f) if f is not None else None), "CopyFiles")
        del keep

    def close(self) -> Primitive:
        self._check(self.lib.pfscdc_fsw_close(self._w), "Close")
        info = _lib.FilesetInfo()
        self._check(self.lib.pfscdc_fsw_fileset(self._w, C.byref(info)), "fileset")
        a = C.string_at(info.additive_root, info.additive_root_len) if info.additive_root else None
        d = C.string_at(info.deletive_root, info.deletive_root_len) if info.deletive_root else None
        return Primitive(a, d, info.size_bytes, info.num_files, info.num_deletes)

    def release(self) -> None:
        """Destroy the writer and hand its data context back to the Storage."""
        if getattr(self, "_w", None):
            self.lib.pfscdc_fsw_destroy(self._w)
            self._w = None
        if getattr(self, "_chunker", None):
            if self._own:
                self._chunker.close()
            else:
                self._storage._give_chunker(self._chunker)
            self._chunker = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class UnorderedWriter:
    def __init__(self, storage: Storage):
        self.lib = _lib.load()
        self._storage = storage
        self._chunker = storage._take_chunker()
        self.events: list = []  # per serialized fileset, its events in arrival order
        self.log: list = []  # every event as (fileset, ...) in arrival order
        self.log_copied: list = []  # per event of log: a data chunk passed through by reference
        self._exc: Optional[BaseException] = None
        # the callback reaches the writer through a weak reference: a bound method here would
        # make a reference cycle, which the cyclic GC frees in arbitrary order, closing the
        # data context before this writer could hand it back to the Storage
        ref = weakref.ref(self)

        def on_event(user, ev_p, _ref=ref):
            o = _ref()
            return o._on_event(user, ev_p) if o is not None else 1

        self._cfun = _lib.UW_CB(on_event)
        ip = storage.index_params.to_c() if storage.index_params else None
        w = C.c_void_p()
        if storage.devices is not None:
            rc = self.lib.pfscdc_uw_create_group(self._chunker.g, storage.mem_threshold,
                                                 C.byref(ip) if ip is not None else None,
                                                 self._cfun, None, C.byref(w))
        else:
            rc = self.lib.pfscdc_uw_create(self._chunker.ctx, storage.mem_threshold,
                                           C.byref(ip) if ip is not None else None, self._cfun,
                                           None, C.byref(w))
        if rc:
            raise _lib.PfsCdcError(rc, "pfscdc_uw_create")
        self._w = w
        if getattr(storage, "store", None) is not None:
            rc = self.lib.pfscdc_uw_set_store(w, storage.store._s)
            if rc:
                raise _lib.PfsCdcError(rc, "pfscdc_uw_set_store")

    def _on_event(self, _user, ev_p) -> int:
        try:
            ev = ev_p.contents
            while len(self.events) <= ev.fileset:
                self.events.append([])
            if ev.kind == _lib.EV_CHUNK:
                ch = ev.chunk
                e = ("chunk", ev.index, ev.level if ev.index >= 0 else 0, ch.size_bytes,
                     bool(ch.edge), bytes(ch.ref.id))
            else:
                e = ("index", ev.index, C.string_at(ev.bytes, ev.len))
            self.events[ev.fileset].append(e)
            self.log.append((ev.fileset,) + e)
            self.log_copied.append(ev.kind == _lib.EV_CHUNK and bool(ev.chunk.copied))
            return 0
        except BaseException as e:
            self._exc = e
            return 1

    def _check(self, rc: int, what: str) -> None:
        if self._exc is not None:
            exc, self._exc = self._exc, None
            raise exc
        if rc:
            msg = self.lib.pfscdc_uw_last_error(self._w) if getattr(self, "_w", None) else None
            raise _lib.PfsCdcError(rc, f"{what}: {msg.decode() if msg else ''}")

    def put(self, p: str, tag: str, append_file: bool, data) -> None:
        arr = np.frombuffer(data, dtype=np.uint8)  # no copy: the library copies once
        self._check(self.lib.pfscdc_uw_put(self._w, p.encode(), tag.encode(), int(append_file),
                                           arr.ctypes.data if arr.size else None, arr.size),
                    "Put")

    def delete(self, p: str, tag: str = "") -> None:
        self._check(self.lib.pfscdc_uw_delete(self._w, p.encode(), tag.encode()), "Delete")

    def copy(self, files: Optional[IndexList], tag: str = "", append: bool = False) -> None:
        """``UnorderedWriter.Copy``: the buffer is serialized, then every entry of ``files`` is
        copied into one more fileset under ``tag`` ("": "default"), each after a Delete of its
        (path, tag) unless ``append``.  Chunks the entries hold whole pass by reference."""
        self._check(self.lib.pfscdc_uw_copy(self._w, files._p if files is not None else None,
                                            tag.encode(), int(append)), "Copy")

    def copy_file(self, src, src_path: str, dst: str, append: bool = False, tag: str = "",
                  src_tag: str = "") -> None:
        """``copyFile``: the file or subtree ``src_path`` of ``src`` under ``dst``.  ``src``: the
        commit's filesets (what ``Storage.open`` takes), opened, selected, mapped and copied in
        one call (pfscdc_uw_copy_file), or an opened ``FileSet``, whose resident list (or host
        list, uploaded) goes through ``copy_map`` and ``copy``."""
        if isinstance(src, FileSet):
            c = Chunker(ChunkParams(), self._storage.device)
            try:
                dev = copy_map(c, src.resident if src.resident is not None else src._list,
                               src_path, dst, src_tag)
                try:
                    mapped = dev.download(c)
                finally:
                    dev.free()
            finally:
                c.close()
            try:
                self.copy(mapped, tag, append)
            finally:
                mapped.free()
            return
        filesets = list(src)
        arr, keep = Storage._infos(filesets)
        self._check(self.lib.pfscdc_uw_copy_file(
            self._w, arr, len(filesets), _path_arg(src_path), _path_arg(src_tag), _path_arg(dst),
            tag.encode(), int(append)), "CopyFile")
        del keep

    def timings(self) -> dict:
        """Stage times (ms) of this writer (pfscdc_uw_timings)."""
        out = (C.c_double * 9)()
        self._check(self.lib.pfscdc_uw_timings(self._w, out), "timings")
        return dict(zip(["put_copy", "upload", "scan", "replay", "hashes", "create",
                         "callbacks", "index", "group_wall"], [round(x, 3) for x in out]))

    def close(self) -> list:
        self._check(self.lib.pfscdc_uw_close(self._w), "Close")
        out = []
        for i in range(self.lib.pfscdc_uw_num_filesets(self._w)):
            info = _lib.FilesetInfo()
            self._check(self.lib.pfscdc_uw_fileset(self._w, i, C.byref(info)), "fileset")
            a = C.string_at(info.additive_root, info.additive_root_len) if info.additive_root else None
            d = C.string_at(info.deletive_root, info.deletive_root_len) if info.deletive_root else None
            out.append(Primitive(a, d, info.size_bytes, info.num_files, info.num_deletes))
        return out

    def release(self) -> None:
        """Destroy the writer and hand its data context back to the Storage."""
        if getattr(self, "_w", None):
            self.lib.pfscdc_uw_destroy(self._w)
            self._w = None
        if getattr(self, "_chunker", None):
            self._storage._give_chunker(self._chunker)
            self._chunker = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
