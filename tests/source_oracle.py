"""An independent restatement of the reference's Source, as the recursion it is.

* ``dir_inserter``  dirInserter.Iterate with emit / parentOf / Clean (fileset/dir_inserter.go:22-58)
* ``index_filter``  indexFilter.Iterate with its ``dir`` state (fileset/transforms.go:31-49)
* ``iterate``       source.Iterate with its cache and its second iterator, computeFileInfo as the
                    recursion over Peek / Next (server/pfs/server/source.go:45-145)
* ``predicate``     the closures getFile / inspectFile / listFile / walkFile hand to the filter
                    (driver_file.go:173-277), globMatchFunction for a literal glob

An entry is ``(path, tag, size, [DataRef hash, ...])``; a stream item ``(path, src)`` with
``src`` the entry's index or None for a dirFile.  ``insert_by_prefix`` and ``infos_by_depth`` are
the data-parallel forms the kernels use, kept here to be held against the literal ones."""
import hashlib

ALL, SUBTREE, LIST, GET = 0, 1, 2, 3
FILE, DIR = 1, 2
CHILD = 1
GLOB_BYTES = "*?[]{}!()@+^\\"


def go_clean(p: str) -> str:
    """path.Clean."""
    if p == "":
        return "."
    rooted = p.startswith("/")
    out = []
    for comp in p.split("/"):
        if comp in ("", "."):
            continue
        if comp == "..":
            if out and out[-1] != "..":
                out.pop()
            elif not rooted:
                out.append("..")
            continue
        out.append(comp)
    s = ("/" if rooted else "") + "/".join(out)
    return s or "."


def is_dir(p: str) -> bool:
    return p.endswith("/")


def fs_clean(p: str, isdir: bool) -> str:
    """fileset.Clean."""
    p = go_clean(p)
    if p == ".":
        return "/"
    y = "/" + p.strip("/")
    if isdir and not is_dir(y):
        y += "/"
    return y


def clean_path(p: str) -> str:
    """The driver's cleanPath."""
    p = go_clean(p)
    if p == ".":
        return "/"
    return "/" + p.strip("/")


def go_dir(p: str) -> str:
    """path.Dir."""
    return go_clean(p[:p.rfind("/") + 1])


def parent_of(x: str) -> str:
    x = x.rstrip("/")
    y = go_dir(x)
    if y == x:
        return "/"
    if not is_dir(y):
        y += "/"
    return y


def _b(s: str) -> bytes:
    return s.encode("utf-8", "surrogateescape")


def dir_inserter(paths):
    """[(path, src)]: the stream dirInserter.Iterate yields for the entries' paths."""
    out = []
    last = [""]

    def emit(p, src):
        parent = fs_clean(parent_of(p), True)
        if p == "/" or _b(last[0]) >= _b(parent):  # Go compares strings bytewise
            out.append((p, src))
            last[0] = p
            return
        emit(parent, None)
        emit(p, src)

    for i, p in enumerate(paths):
        emit(p, i)
    return out


def insert_by_prefix(paths):
    """The same for clean paths in ascending order, entry by entry: the ancestors p[:k + 1]
    with p[k] == '/', k < len - 1 and k >= the common-prefix length with the entry before."""
    out = []
    for i, p in enumerate(paths):
        pb = _b(p)
        lcp = 0
        if i:
            qb = _b(paths[i - 1])
            while lcp < min(len(pb), len(qb)) and pb[lcp] == qb[lcp]:
                lcp += 1
        for k in range(lcp, len(pb) - 1):
            if pb[k] == 0x2F:
                out.append((pb[:k + 1].decode("utf-8", "surrogateescape"), None))
        out.append((p, i))
    return out


def predicate(kind: int, arg: str):
    """(match function, full) as the RPC builds them; ValueError for a glob pattern."""
    if kind == ALL:
        return (lambda path: True), False
    if kind == SUBTREE:
        p = clean_path(arg)
        if p == "/":
            p = ""
        return (lambda path: path == p or path.startswith(p + "/")), False
    if kind == LIST:
        name = clean_path(arg)

        def match(path):
            if path == fs_clean(name, True):
                return False
            if path == name:
                return True
            return path.startswith(fs_clean(name, True))
        return match, False
    glob = clean_path(arg)
    if any(c in glob for c in GLOB_BYTES):
        raise ValueError(glob)

    def mf(path):  # globMatchFunction with a glob that matches only itself
        if path == "/" and glob == "/":
            return True
        return path.rstrip("/") == glob
    return mf, True


def index_filter(stream, match, full):
    out = []
    d = ""
    for path, src in stream:
        if full:
            if d != "" and path.startswith(d):
                out.append((path, src))
                continue
            if match(path) and is_dir(path):
                d = path
        if match(path):
            out.append((path, src))
    return out


def path_is_child(parent: str, child: str) -> bool:
    if not child.startswith(parent):
        return False
    return "/" not in child[len(parent):].strip("/")


class StreamError(Exception):
    """source.Iterate's own errors: the second iterator is not where the first one is (paths
    that are not clean can bring that about)."""


def hash_data_refs(hashes) -> bytes:
    h = hashlib.blake2b(digest_size=32)
    for x in hashes:
        h.update(x)
    return h.digest()


def iterate(stream, entries, leaf=None):
    """[(size, hash)] per item of ``stream``, as source.Iterate computes them."""
    pos = [0]  # fileset.NewIterator(ctx, s.fileSet)
    cache = {}

    def regular(item):
        path, src = item
        assert src is not None, "Hash of a dirFile"
        _, _, size, hashes = entries[src]
        return size, (leaf[src] if leaf is not None else hash_data_refs(hashes))

    def compute(target):
        if pos[0] >= len(stream):
            raise StreamError("stream is done, can't compute hash for " + target)
        item = stream[pos[0]]
        pos[0] += 1
        if item[0] != target:
            raise StreamError("stream is wrong place to compute hash for " + target)
        if not is_dir(item[0]):
            return regular(item)
        size = 0
        h = hashlib.blake2b(digest_size=32)
        while pos[0] < len(stream) and stream[pos[0]][0].startswith(target):
            csize, chash = compute(stream[pos[0]][0])
            size += csize
            h.update(chash)
        size = (size + (1 << 63)) % (1 << 64) - (1 << 63)  # int64 wraps
        cache[target] = (size, h.digest())
        return cache[target]

    out = []
    for item in stream:
        path = item[0]
        if path in cache:
            out.append(cache[path])
        elif path[:path.rfind("/") + 1] in cache:  # path.Split
            out.append(regular(item))
        else:
            out.append(compute(path))
    return out


def infos_by_depth(stream, entries, leaf=None):
    """The same without the iterator: a directory's subtree is the run of paths with its prefix
    after it, its children the entries of the next depth in that run."""
    n = len(stream)
    depth = [_b(p)[:-1].count(b"/") for p, _ in stream]
    res = [None] * n
    for o, (p, src) in enumerate(stream):
        if not is_dir(p):
            _, _, size, hashes = entries[src]
            res[o] = (size, leaf[src] if leaf is not None else hash_data_refs(hashes))
    for level in range(max(depth, default=-1), -1, -1):
        for o, (p, _) in enumerate(stream):
            if depth[o] != level or not is_dir(p):
                continue
            end = o + 1
            while end < n and stream[end][0].startswith(p):
                end += 1
            kids = [res[c] for c in range(o + 1, end) if depth[c] == level + 1]
            size = sum(res[c][0] for c in range(o + 1, end) if not is_dir(stream[c][0]))
            size = (size + (1 << 63)) % (1 << 64) - (1 << 63)
            res[o] = (size, hash_data_refs(h for _, h in kids))
    return res


def source(entries, kind: int, arg: str = "", leaf=None):
    """The whole Source: [(path, tag, src, type, size, hash, flags)], or KeyError where
    NewErrOnEmpty answers, ValueError for a glob pattern."""
    match, full = predicate(kind, arg)
    stream = index_filter(dir_inserter([e[0] for e in entries]), match, full)
    infos = iterate(stream, entries, leaf)
    name = clean_path(arg)
    out = []
    for (path, src), (size, h) in zip(stream, infos):
        flags = CHILD if kind == LIST and path_is_child(name, clean_path(path)) else 0
        out.append((path, entries[src][1] if src is not None else "", src,
                    DIR if is_dir(path) else FILE, size, h, flags))
    if not out and (kind == GET or (kind == SUBTREE and clean_path(arg) != "/")):
        raise KeyError(arg)
    return out
