"""The lists and predicates the Source tests share (CPU: pfscdc_source_host against
tests/source_oracle.py; GPU: pfscdc_source_open against pfscdc_source_host), and the
comparison of a result with the oracle's."""
import random

from oracle import chunker as Ch
from oracle import fileset as OF
from pfs_amd import _lib
from pfs_amd import fileset as pf

import source_oracle as SO

KINDS = (SO.ALL, SO.SUBTREE, SO.LIST, SO.GET)
# a file, a directory, both a file /a and a directory /a/, nothing, "/", "", a byte-prefix of a
# sibling (/a beside /ab), an unclean spelling
ARGS = ("", "/", "/a", "/a/", "/a/b", "/a/c", "/a/c/d", "/ab", "/nothing", "a/./c/../c", "/a/b!")


def dr(rng, size=None):
    ref = Ch.Ref(size_bytes=1 << 62, edge=False, id=rng.randbytes(32), dek=rng.randbytes(32))
    return Ch.DataRef(ref, rng.randbytes(32), rng.randrange(1 << 20),
                      rng.randrange(1 << 20) if size is None else size)


def build(rng, spec):
    """``spec``: [(path, tag, number of DataRefs or their sizes)] in list order.  Returns the
    oracle's entries [(path, tag, size, [hash])] and the decoded IndexList."""
    idx = []
    for path, tag, drs in spec:
        sizes = [None] * drs if isinstance(drs, int) else drs
        idx.append(OF.Index(path, tag, [dr(rng, s) for s in sizes]))
    lst = pf.index_decode_host(b"".join(OF.frame(OF.encode_index(e)) for e in idx))
    entries = []
    for e in idx:
        size = sum(d.size_bytes for d in e.data_refs)
        size = (size + (1 << 63)) % (1 << 64) - (1 << 63)
        entries.append((e.path, e.tag, size, [bytes(d.hash) for d in e.data_refs]))
    return entries, lst, idx


def by_key(spec):
    return sorted(spec, key=lambda e: (e[0].encode(), e[1].encode()))


def hand_trees():
    """name -> spec.  Siblings that straddle '/' in byte order, a deep chain, two tags of one
    path, 0 / 1 / 300 DataRefs, an explicit directory entry, sizes that wrap int64, the empty
    list."""
    straddle = by_key([(p, "t", 1) for p in
                       ("/a!x", "/a-c/d", "/a.x", "/a/b", "/a/c/d", "/a0", "/a/b!/d", "/a/b/c",
                        "/a", "/ab", "/a/c/e")])
    return {
        "straddle": straddle,
        "chain12": [("/" + "/".join("d%d" % i for i in range(12)) + "/leaf", "t", 2)],
        "two_tags": by_key([("/a/f", "x", 1), ("/a/f", "y", 2), ("/a/g", "x", 0), ("/b", "", 1)]),
        "refs_0_1_300": [("/a/r0", "t", 0), ("/a/r1", "t", 1), ("/a/r300", "t", 300)],
        "explicit_dir": [("/a/", "", 0), ("/a/b", "t", 1), ("/a/c/", "", 0), ("/a/c/d", "t", 1),
                         ("/e/", "", 0)],
        "wrap": [("/a/w0", "t", [1 << 62, 1 << 62]), ("/a/w1", "t", [1 << 62, (1 << 62) + 5]),
                 ("/b", "t", [7])],
        "root_only": [("/", "", 0)],
        "empty": [],
    }


def host_only_trees():
    """Lists the device arm hands to the host arm: unsorted, unclean paths, a directory twice."""
    return {
        "unsorted": [("/b", "t", 1), ("/a/x", "t", 1), ("/a/y", "t", 1)],
        "unclean_slashes": [("//x", "t", 1), ("/y", "t", 1)],
        "unclean_rel": [("/a", "t", 1), ("rel", "t", 1)],
        "unclean_dot": [("/a/./b", "t", 1), ("/a/c", "t", 1)],
        "dir_twice": [("/a/", "x", 0), ("/a/", "y", 0), ("/a/b", "t", 1)],
    }


def random_tree(rng, n=None):
    comps = ["a", "b", "ab", "a!", "a-", "a.", "a0", "c", "d"]
    n = rng.randrange(1, 30) if n is None else n
    seen, spec = set(), []
    while len(spec) < n:
        depth = rng.choice([1, 1, 2, 2, 3, 4])
        path = "/" + "/".join(rng.choice(comps) for _ in range(depth))
        if rng.random() < 0.08:
            path, tag = path + "/", ""  # an explicit directory entry
            if any(p == path for p, _ in seen):
                continue
        else:
            tag = rng.choice(["", "t", "t", "u"])
        if (path, tag) in seen:
            continue
        seen.add((path, tag))
        spec.append((path, tag, rng.choice([0, 1, 1, 2, 3])))
    return by_key(spec)


def sequence(n):
    """n files over a small tree, in order (for the input-length cases)."""
    return by_key([("/s%02d/f%05d" % (i % 7, i), "t", 1 if i % 5 else 0) for i in range(n)])


def leaf_of(n):
    """Caller-supplied leaf hashes: 32 bytes per entry."""
    return [bytes((i * 7 + k * 3 + 1) & 0xFF for k in range(32)) for i in range(n)]


def want(entries, kind, arg, leaf=None):
    """The oracle's answer: ("ok", rows), ("notfound",), ("unsupported",), or ("error",) where
    source.Iterate itself fails."""
    try:
        return ("ok", SO.source(entries, kind, arg, leaf))
    except KeyError:
        return ("notfound",)
    except ValueError:
        return ("unsupported",)
    except SO.StreamError:
        return ("error",)


def got_host(lst, kind, arg, leaf=None):
    try:
        res, infos = pf.source_host(lst, kind, arg, b"".join(leaf) if leaf is not None else None)
    except KeyError:
        return ("notfound",), None
    except _lib.PfsCdcError as e:
        assert e.code in (_lib.PFSCDC_EUNSUPPORTED, _lib.PFSCDC_EINVAL), e
        return ("unsupported" if e.code == _lib.PFSCDC_EUNSUPPORTED else "error",), None
    return ("ok", rows_of(res, infos)), res


def rows_of(res, infos):
    """A result as the oracle's rows, src left out: (path, tag, type, size, hash, flags,
    DataRef hashes)."""
    rows = []
    n, ents, _, _, ndr = res._views()
    at = 0
    for i, (d, (h, size, typ, flags)) in enumerate(zip(res.raw(), infos)):
        assert d["has_file"] and d["range"] is None
        assert ents[i].first == at, "first is packed in entry order"
        at += ents[i].count
        rows.append((d["path"].decode("utf-8", "surrogateescape"),
                     d["tag"].decode("utf-8", "surrogateescape"), typ, size, h, flags,
                     [bytes(x.hash) for x in d["data_refs"]]))
    assert at == ndr and n == len(infos)
    return rows


def rows_want(w, entries):
    return [(p, t, typ, size, h, flags, entries[src][3] if src is not None else [])
            for p, t, src, typ, size, h, flags in w]


def check_against_oracle(entries, lst, kind, arg, leaf=None):
    w = want(entries, kind, arg, leaf)
    g, _ = got_host(lst, kind, arg, leaf)
    assert g[0] == w[0], (kind, arg, g[0], w[0])
    if w[0] == "ok":
        assert g[1] == rows_want(w[1], entries), (kind, arg)
    return w
