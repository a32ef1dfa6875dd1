"""Differ.Iterate (src/server/pfs/server/diff.go:26-96) restated in Python: the two-pointer walk
over two sides, each a list of (path, hash) rows in the order its Source yields them.  Paths
compare as Go strings do (unsigned bytes, a proper prefix first); the tag is no part of the key;
equal paths advance both sides and are reported only if the hashes differ (equalFileInfos); both
tails are drained.  Nothing here assumes sorted sides: the walk does what it does."""
import random

import source_cases as SC


def _key(path):
    return path.encode("utf-8", "surrogateescape") if isinstance(path, str) else bytes(path)


def diff(a, b):
    """[(i or None, j or None)] per callback, in callback order: indexes into ``a`` and ``b``."""
    out, i, j = [], 0, 0
    while i < len(a) and j < len(b):
        pa, pb = _key(a[i][0]), _key(b[j][0])
        if pa < pb:
            out.append((i, None))
            i += 1
        elif pb < pa:
            out.append((None, j))
            j += 1
        else:
            if bytes(a[i][1]) != bytes(b[j][1]):
                out.append((i, j))
            i += 1
            j += 1
    out += [(k, None) for k in range(i, len(a))]
    out += [(None, k) for k in range(j, len(b))]
    return out


# ---- sides for the tests: a spec of source_cases.build with one hash per entry

def hash_of(seed):
    return random.Random(seed).randbytes(32)


def side(rng, rows):
    """``rows``: [(path, tag, hash)] in list order.  The decoded IndexList with one DataRef per
    file, the infos pfscdc_diff_host takes and the oracle's (path, hash) rows."""
    _, lst, _ = SC.build(rng, [(p, t, 0 if p.endswith("/") else 1) for p, t, _ in rows])
    infos = [(bytes(h), 7 * k, 2 if p.endswith("/") else 1, 0) for k, (p, _, h) in enumerate(rows)]
    return (lst if rows else None), infos, [(p, h) for p, _, h in rows]


def changed(rng, rows, drop=0.1, add=0.1, rehash=0.2):
    """Side b from side a: entries dropped, added and re-hashed, in path-then-tag order."""
    out = []
    for p, t, h in rows:
        r = rng.random()
        if r < drop:
            continue
        out.append((p, t, rng.randbytes(32) if r < drop + rehash else h))
    have = {(p, t) for p, t, _ in out}
    for _ in range(int(add * len(rows)) + rng.randrange(3)):
        p = rng.choice([r[0] for r in rows] + ["/n"]) + rng.choice(["", "!", "0", "/n", "x"])
        if p.endswith("/") or "//" in p:
            continue
        t = rng.choice(["", "t", "u", "v"])
        if (p, t) not in have:
            have.add((p, t))
            out.append((p, t, rng.randbytes(32)))
    return sorted(out, key=lambda r: (r[0].encode(), r[1].encode()))
