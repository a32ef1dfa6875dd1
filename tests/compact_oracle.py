"""Storage.Compact restated over the oracle (test helper, no GPU): oracle.fileset.FilesetWriter
with Copy (fileset/writer.go:105-125) over the oracle chunk writer's Copy against a dict store,
MergeReader.iterate / iterateDeletive by sort and group, and CopyFiles (util.go:27-40)."""
import copy

from oracle import chunker as Ch
from oracle import fileset as OF
from test_index_read_cpu import merge_restated


class CopyChunkWriter(OF._ChunkWriter):
    """The data stream's chunk writer with the chunk client: Copy reads chunks from ``store``
    (Ref.Id -> ciphertext), new chunks are uploaded into it, and a chunk passed through by
    reference is logged as a chunk event with copied = True."""

    def __init__(self, params, cb, log, stream, store):
        super().__init__(params, cb, log, stream)
        self.store = store

    def _process_chunk(self, chunk, edge, annotations):
        super()._process_chunk(chunk, edge, annotations)
        self.log[-1] = self.log[-1] + (False,)

    def _maybe_cheap_copy(self):                             # writer.go:403-420
        last = self.annotations[-1].next_data_ref if self.buffering else None
        super()._maybe_cheap_copy()
        if last is not None and not self.buffering:
            self.log.append(("chunk",) + self.stream +
                            (last.ref.size_bytes, last.ref.edge, last.ref.id, True))


class CopyFilesetWriter(OF.FilesetWriter):
    def __init__(self, params, log, index_params, store):
        super().__init__(params, log, index_params)
        self.cw = CopyChunkWriter(params, self._callback, log, (-1, 0), store)

    def copy(self, path, tag, data_refs):                    # writer.go:105-125
        idx = OF.Index(path=path, tag=tag)
        self._check_path(self.idx, idx)
        self.idx = idx
        self.files.append((path, tag))
        self.cw.annotate(Ch.Annotation(data=idx))
        for d in data_refs:
            self.size_bytes += d.size_bytes
            self.cw.copy(copy.deepcopy(d))


def deletive_restated(filesets):
    """iterateDeletive (merge.go:79-94): per (path, tag) of the deletive lists, once."""
    return sorted({(p, t) for dele, _ in filesets for p, t, _ in dele})


def compact(filesets, params, index_params, store):
    """filesets: [(deletive, additive)] lists of (path, tag, [Ch.DataRef]) (bytes paths), in
    fileset order.  Returns (Primitive, log).  Storage.Open: one fileset is not merged."""
    log = []
    w = CopyFilesetWriter(params, log, index_params, store)
    if len(filesets) == 1:
        deletes = [(p, t) for p, t, _ in filesets[0][0]]
        files = filesets[0][1]
    else:
        deletes = deletive_restated(filesets)
        files = merge_restated(filesets)
    for p, t in deletes:                                     # CopyFiles(ctx, w, fs, true)
        w.delete(p.decode(), t.decode())
    for p, t, drs in files:
        w.copy(p.decode(), t.decode(), drs)
    return w.close(), log
