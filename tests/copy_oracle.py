"""CopyFile restated over the oracle (test helper, no GPU): cleanPath, the open's options, the
filter and the mapper of driver.copyFile (server/pfs/server/driver_file.go:143-171, paths.go:54-60,
fileset/transforms.go:20-90, index/reader.go:95-122), and UnorderedWriter.Copy
(fileset/unordered_writer.go:151-168) with its interleaved Delete and Copy over
compact_oracle.CopyFilesetWriter.  Go's path.Clean, path.Join and filepath.Rel lean on posixpath,
which differs from Go in one point only: normpath keeps a leading "//"."""
import posixpath

from oracle import fileset as OF

import compact_oracle as CO


def go_clean(p: str) -> str:
    """path.Clean."""
    if p == "":
        return "."
    r = posixpath.normpath(p)
    return r[1:] if r.startswith("//") else r


def clean_path(p: str) -> str:
    """cleanPath (paths.go:54-60)."""
    p = go_clean(p)
    if p == ".":
        return "/"
    return "/" + p.strip("/")


def go_rel(base: str, targ: str) -> str:
    """filepath.Rel on Unix, for two rooted paths (the only ones copyFile hands it)."""
    base, targ = go_clean(base), go_clean(targ)
    assert base.startswith("/") and targ.startswith("/")
    return posixpath.relpath(targ, base)


def go_join(a: str, b: str) -> str:
    """path.Join of two elements."""
    parts = [x for x in (a, b) if x != ""]
    return go_clean("/".join(parts)) if parts else ""


def _b(s: str) -> bytes:
    return s.encode("utf-8", "surrogateescape")


def copy_map(entries, src: str, dst: str, src_tag: str = ""):
    """entries: [(path, tag, ...)] in list order.  The (index into entries, new path) pairs
    copyFile hands to UnorderedWriter.Copy, in order."""
    src_path, dst_path = clean_path(src), clean_path(dst)
    prefix = _b(src_path)
    out = []
    for i, e in enumerate(entries):
        path, tag = e[0], e[1]
        name = _b(path)
        # Reader.Iterate with index.WithPrefix(srcPath), index.WithTag(src.Tag)
        k = min(len(name), len(prefix))
        if name[:k] > prefix[:k]:        # atEnd
            break
        if not name >= prefix:           # atStart
            continue
        if not (src_tag == "" or src_tag == tag):
            continue
        # NewIndexFilter
        if not (path == src_path or name.startswith(_b(src_path + "/"))):
            continue
        # NewIndexMapper: pathTransform
        out.append((i, go_join(dst_path, go_rel(src_path, path))))
    return out


class CopyUnorderedWriter(OF.UnorderedWriter):
    """The oracle's UnorderedWriter with Copy; ``store``: Ref.Id -> ciphertext of the chunks the
    copied files lie in (Copy reads the ones it re-rolls from it)."""

    def __init__(self, params, mem_threshold, index_params, store):
        super().__init__(params, mem_threshold, index_params)
        self.store = store

    def copy(self, files, tag: str = "", append_file: bool = False) -> None:
        """files: [(path, [Ch.DataRef])] in order (unordered_writer.go:151-168)."""
        self.serialize()
        if tag == "":
            tag = OF.DEFAULT_FILE_TAG
        log: list = []
        w = CO.CopyFilesetWriter(self.params, log, self.index_params, self.store)  # withWriter
        for path, data_refs in files:
            if not append_file:
                w.delete(path, tag)
            w.copy(path, tag, data_refs)
        self.filesets.append(w.close())
        self.log.append(log)
        self.buffer = OF.Buffer()
        self.mem_available = self.mem_threshold
