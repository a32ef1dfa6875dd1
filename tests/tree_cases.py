"""One large irregular tree for the tree passes (Source, GlobFile, DiffFile, CopyFile's map): a
few thousand entries whose neighbours differ in common-prefix length, depth, name length and
tag count all at once, with bytes >= 0x80 and directory paths past 256 bytes, so that every lane
of a pass sees another situation than the lane beside it.

``irregular_tree`` returns a spec as ``source_cases.build`` takes it.  The parts:

* a spine of ``spine`` nested directories, their names cycling through ``POOL`` but for "a!",
  with a file ``f`` on every level: the deepest path has ``spine + 1`` '/';
* ``WIDE`` (depth 4) with ``wide`` immediate children from several stems, every 11th of them a
  directory and every 13th a file of two tags;
* ``bushes`` sibling directories ``BUSHES/kNNNN`` at depth 3 with 1-3 files each, a fifth of
  them with a sub-directory ``sub``: level 3 holds more than 1,024 directories and level 4 more
  than 1,024 entries;
* ``extra`` random paths of depth 1-9 over ``POOL``, a tenth with a second tag, some with four,
  one in twenty an explicit directory entry (never under /a or /b, so CopyFile's map keeps the
  device arm for the sources below them: a selected directory entry is not clean as a file path);
* 0-3 DataRefs per file and one file with 300;
* ``shift`` files ``/!padNNNN`` in front of everything, which move every later input and output
  index by ``shift``.
"""
import functools
import random

import diff_oracle as DO
import source_cases as SC
import source_oracle as SO

LONG = "l" + "o" * 88 + "g"  # 90 bytes
# byte-order straddlers around '/', two names with bytes >= 0x80, the long one, and z~
POOL = ["a", "ab", "a!", "a-", "a.", "a0", "é", "日本", LONG, "z~"]
WIDE = "/a/a!/a-/w"
BUSHES = "/b/ab"
BUSH = BUSHES + "/k0517"  # one bush with a sub-directory (517 % 5 == 2)
NOT_THERE = "/a/ab/nothing"

# the tree's own globs ('!' is extglob outside a class, so it is escaped)
GLOBS = ("/**", "/b/ab/k0*/**", "/**/f", "/a/a\\!/a-/w/f\\!*", "/b/*/k1???/*1", "/{a,b}/**0",
         "/*/*", "/**/sub/*", "/[é日]*/**")


def spine_dirs(spine):
    """The spine's directories without the trailing '/', outermost first."""
    names = [c for c in POOL if c != "a!"]  # getFile takes a path with '!' for a pattern
    out, p = [], ""
    for k in range(spine):
        p += "/" + names[k % len(names)]
        out.append(p)
    return out


def irregular_tree(rng, spine, wide=1030, bushes=1030, extra=300, shift=0):
    seen, spec = set(), []

    def add(path, tag, drs):
        if (path, tag) in seen:
            return False
        seen.add((path, tag))
        spec.append((path, tag, drs))
        return True

    def refs():
        return rng.choice([0, 1, 1, 2, 3])

    for d in spine_dirs(spine):
        add(d + "/f", "t", refs())
    stems = ("f!%04d", "f%04d", "g-%04d", "é%04d", "a.%04d", "日%04d")
    for i in range(wide):
        name = WIDE + "/" + rng.choice(stems) % i
        if i % 11 == 5:
            add(name + "/x", "t", refs())  # a directory among the children
            if i % 2:
                add(name + "/é/y", "u", refs())
        else:
            add(name, "t", refs())
            if i % 13 == 3:
                add(name, "u", refs())
    add(WIDE + "/r300", "t", 300)
    for i in range(bushes):
        bush = "%s/k%04d" % (BUSHES, i)
        for name in rng.sample(["x1", "y0", "é1", "a!0", "zz", "a.1"], rng.randrange(1, 4)):
            add(bush + "/" + name, "t", refs())
            if rng.random() < 0.04:
                add(bush + "/" + name, "u", refs())
        if i % 5 == 2:
            for name in rng.sample(["n", "m0", "日"], rng.randrange(1, 3)):
                add(bush + "/sub/" + name, "t", refs())
    dirs, n = set(), 0
    while n < extra:
        depth = rng.randrange(1, 10)
        path = "/" + "/".join(rng.choice(POOL) for _ in range(depth))
        r = rng.random()
        if r < 0.05:
            # an explicit directory entry: once per directory, and not under /a or /b
            if path.split("/")[1] in ("a", "b") or path in dirs:
                continue
            dirs.add(path)
            n += add(path + "/", "", 0)
            continue
        tags = ("t", "u") if r < 0.15 else ("", "t", "u", "v") if r < 0.18 else (rng.choice(["", "t", "u"]),)
        for tag in tags:
            n += add(path, tag, refs())
    for k in range(shift):
        add("/!pad%04d" % k, "t", 1)
    return SC.by_key(spec)


def depth_of(path):
    """The '/' in a path but a trailing one: "/" is 0, /a and /a/ are 1."""
    return SO._b(path)[:-1].count(b"/")


def source_args(spine):
    """The arguments of SUBTREE / LIST / GET: the wide directory, the bushes' parent, one bush,
    the spine's deepest directory, the root, a path that is not there."""
    return (WIDE, BUSHES, BUSH, spine_dirs(spine)[-1], "/", NOT_THERE)


def copy_pairs(spine):
    """(src, dst, src_tag): the bushes' parent to /z/y, the wide directory to the root, /a to a
    destination inside it, one bush to /q, one tag of the wide directory, nothing."""
    return ((BUSHES, "/z/y", ""), (WIDE, "/", ""), ("/a", "/a/a!", ""), (BUSH, "/q", ""),
            (WIDE, "/日本/w", "u"), (NOT_THERE, "/z", ""))


def first_shift(ok, limit=64):
    """The least p < limit with ok(p), or None."""
    return next((p for p in range(limit) if ok(p)), None)


def dir_edge_shift(stream, edge=1024):
    """``stream``: the unshifted tree's dir_inserter output [(path, src)].  The shift p under
    which output entry edge - 1 is an inserted directory and entry edge its first child ("/"
    stays entry 0 and the p pads follow it, so every other entry moves by p)."""
    def ok(p):
        o = edge - 1 - p
        return 0 < o < len(stream) - 1 and stream[o][1] is None and \
            stream[o + 1][0].startswith(stream[o][0])
    return first_shift(ok)


def tag_edge_shift(paths, edge=1024):
    """``paths``: the unshifted list's paths in order.  The shift p under which entries
    edge - 1 and edge are two tags of one path."""
    def ok(p):
        return edge - p < len(paths) and edge - 1 - p >= 0 and paths[edge - 1 - p] == paths[edge - p]
    return first_shift(ok)


# ---- built once per process and shared by the CPU and the GPU tests; nothing changes them

@functools.lru_cache(maxsize=None)
def built(spine, shift=0):
    """(spec, the oracle's entries, the decoded IndexList, the Index records) of the tree; the
    shifted trees are the same tree behind their pads."""
    spec = irregular_tree(random.Random(1000 + spine), spine, shift=shift)
    entries, lst, idx = SC.build(random.Random(spine), spec)
    return spec, entries, lst, idx


@functools.lru_cache(maxsize=None)
def oracle_all(spine, shift=0):
    """The oracle's rows of SRC_ALL over the tree."""
    return SO.source(built(spine, shift)[1], SO.ALL, "")


@functools.lru_cache(maxsize=None)
def shifts(spine):
    """(the shift that puts an inserted directory and its first child on output entries 1,023
    and 1,024; the one that puts two tags of one path on input entries 1,023 and 1,024; the one
    that puts them on output entries 1,023 and 1,024, where DiffFile reads them)."""
    return (dir_edge_shift([(r[0], r[2]) for r in oracle_all(spine)]),
            tag_edge_shift([e[0] for e in built(spine)[1]]),
            tag_edge_shift([r[0] for r in oracle_all(spine)]))


class Side:
    """One side of a diff: ``rows`` [(path, tag, hash)] in list order, the list with one DataRef
    per file, the hashes as leaf hashes, and the oracle's Source rows over them."""

    def __init__(self, rows, seed):
        self.rows = rows
        self.entries, self.lst, self.idx = SC.build(
            random.Random(seed), [(p, t, 0 if p.endswith("/") else 1) for p, t, _ in rows])
        self.leaf = b"".join(h for _, _, h in rows)
        self.source = SO.source(self.entries, SO.SUBTREE, "", [h for _, _, h in rows])


@functools.lru_cache(maxsize=None)
def diff_sides(spine, shift=0):
    """Side a: the tree with a hash per entry.  Side b: ``diff_oracle.changed`` of it (a tenth
    dropped, a tenth added, a fifth re-hashed), and the spine's deepest file re-hashed whatever
    was drawn for it, so every directory of the spine and the root change with it."""
    rng = random.Random(7000 + spine)
    ra = [(p, t, rng.randbytes(32)) for p, t, _ in built(spine, shift)[0]]
    deepest = spine_dirs(spine)[-1] + "/f"
    rb = [r for r in DO.changed(rng, ra) if r[0] != deepest] + [(deepest, "t", rng.randbytes(32))]
    rb.sort(key=lambda r: (SO._b(r[0]), SO._b(r[1])))
    return Side(ra, 1), Side(rb, 2)
