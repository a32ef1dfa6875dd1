"""The lists and arguments the CopyFile tests share (CPU: pfscdc_copy_map_host against
tests/copy_oracle.py; GPU: pfscdc_dev_list_copy_map against pfscdc_copy_map_host), and the
comparison of a mapped list with the oracle's."""
import random

import copy_oracle as CPO
import source_cases as SC

LONG = "/a/" + "d" * 296 + "x"  # 300 bytes


def table():
    """name -> (spec, src, dst, src_tag, clean): spec as source_cases.build takes it; clean: every
    selected path is clean as a file path and the list is in order (the device arm takes it)."""
    nb = SC.by_key([(p, "t", k % 3) for k, p in enumerate(("/a", "/a.txt", "/a/x", "/a/y/z", "/ab"))])
    two = SC.by_key([("/a/f", "x", 1), ("/a/f", "y", 2), ("/a/g", "x", 0), ("/a/g", "y", 1),
                     ("/b", "x", 1)])
    return {
        # /a.txt sorts between /a and /a/x: two separate runs are selected
        "neighbours": (nb, "/a", "/z", "", True),
        "single_file": (nb, "/a/y/z", "/q/r", "", True),
        "single_file_to_root": (nb, "/a/x", "/", "", True),
        "cleaning": (nb, "a/", "z/", "", True),
        "cleaning_dots": (nb, "/b/../a/./", "//z//w/..", "", True),
        "dst_root": (nb, "/a", "/", "", True),
        "src_root": (nb, "/", "/z", "", True),
        "src_is_dst": (nb, "/a", "/a", "", True),
        "src_absent": (nb, "/nothing", "/z", "", True),
        "src_below_all": (nb, "/A", "/z", "", True),
        "src_tag_x": (two, "/a", "/z", "x", True),
        "src_tag_y": (two, "/a/f", "/f2", "y", True),
        "src_tag_none": (two, "/a", "/z", "w", True),
        "two_tags_all": (two, "/a", "/z", "", True),
        "unclean_trailing": ([("/a/w", "t", 1), ("/a/x/", "t", 1), ("/a/y", "t", 2)], "/a", "/z", "", False),
        "unclean_dotdot": ([("/a/../b", "t", 1), ("/a/c", "t", 1)], "/a", "/z/y", "", False),
        "unclean_dotdot_root": ([("/a/../b", "t", 1), ("/a/c", "t", 1)], "/a", "/", "", False),
        "unclean_unselected": ([("/a/c", "t", 1), ("/b/./c", "t", 1), ("/c//d", "t", 2)], "/a", "/z", "", True),
        "root_entry": ([("/", "", 0), ("/a", "t", 1)], "/", "/z", "", False),
        "double_slash": ([("//x", "t", 1), ("/y", "t", 1)], "/", "/z", "", False),
        "long_path": (SC.by_key([(LONG, "t", 2), ("/a/b", "t", 1), (LONG[:-1] + "y", "t", 1)]),
                      "/a", "/" + "z" * 290, "", True),
        "long_src": (SC.by_key([(LONG, "t", 2), (LONG + "/k", "t", 1)]), LONG, "/s", "", True),
        "refs_0_1_300": ([("/a/r0", "t", 0), ("/a/r1", "t", 1), ("/a/r300", "t", 300)], "/a", "/z", "", True),
        "unsorted": ([("/b", "t", 1), ("/a/x", "t", 1), ("/a/y", "t", 1)], "/a", "/z", "", False),
        "unsorted_tags": ([("/a/x", "u", 1), ("/a/x", "t", 1)], "/a", "/z", "", False),
        "empty": ([], "/a", "/z", "", True),
    }


def random_list(rng, n):
    """n entries over a small tree in (path, tag) order, two tags on some paths."""
    comps = ["a", "b", "ab", "a.", "a0", "c"]
    seen, spec = set(), []
    while len(spec) < n:
        depth = rng.choice([1, 2, 2, 3, 3, 4])
        path = "/" + "/".join(rng.choice(comps) + str(rng.randrange(4)) for _ in range(depth))
        for tag in (("t", "u") if rng.random() < 0.25 else (rng.choice(["t", "u", ""]),)):
            if (path, tag) not in seen and len(spec) < n:
                seen.add((path, tag))
                spec.append((path, tag, rng.choice([0, 1, 1, 2, 3])))
    return SC.by_key(spec)


def every_second(n, width=5):
    """n entries, every second one under /s: /s/f00000, /t00001, /s/f00002, ... sorted."""
    return SC.by_key([("/s/f%0*d" % (width, i) if i % 2 == 0 else "/t%0*d" % (width, i), "t",
                       1 if i % 3 else 0) for i in range(n)])


def rows(lst):
    """A list as comparable rows: (path, tag, size, has_file, [DataRef fields])."""
    n, ents, _, _, ndr = lst._views()
    out, at = [], 0
    for i, d in enumerate(lst.raw()):
        assert d["range"] is None
        assert ents[i].first == at, "first is packed in entry order"
        assert ents[i].last_path_len == 0
        at += ents[i].count
        out.append((d["path"].decode("utf-8", "surrogateescape"),
                    d["tag"].decode("utf-8", "surrogateescape"), d["size_bytes"], d["has_file"],
                    [(x.ref.id, x.ref.dek, x.ref.size_bytes, x.ref.edge, x.hash, x.offset_bytes,
                      x.size_bytes) for x in d["data_refs"]]))
    assert at == ndr
    return out


def want_rows(lst, src, dst, src_tag=""):
    """The oracle's answer over the decoded input list: the selected rows with their new paths."""
    r = rows_unpacked(lst)
    return [(np,) + r[i][1:] for i, np in CPO.copy_map(r, src, dst, src_tag)]


def rows_unpacked(lst):
    """rows() of an input list, whose DataRefs need not be packed."""
    return [(d["path"].decode("utf-8", "surrogateescape"),
             d["tag"].decode("utf-8", "surrogateescape"), d["size_bytes"], d["has_file"],
             [(x.ref.id, x.ref.dek, x.ref.size_bytes, x.ref.edge, x.hash, x.offset_bytes,
               x.size_bytes) for x in d["data_refs"]]) for d in lst.raw()]


def arrays(lst):
    """The three arrays of a list as bytes, for array-for-array comparisons."""
    import ctypes as C
    from pfs_amd import _lib
    n, ents, blob, drs, ndr = lst._views()
    return (C.string_at(ents, C.sizeof(_lib.IndexEntry) * n) if n else b"", blob,
            C.string_at(drs, C.sizeof(_lib.FullDataRef) * ndr) if ndr else b"")


def build(spec, seed=0):
    rng = random.Random(seed)
    _, lst, idx = SC.build(rng, spec)
    return lst, idx
