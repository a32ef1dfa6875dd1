"""An independent restatement of the glob dialect of getFile / globFile ("GlobFile"),
twice: a parser with a backtracking matcher, and a translation of the glob's text to ``re``.
Both work on bytes.  On top of them the two RPCs as the reference builds them
(server/pfs/server/paths.go:12-35, driver_file.go:173-193 and :284-308) over the literal
pipeline of tests/source_oracle.py, and the stateless form of the ``full`` filter the device
uses.

The dialect (gobwas/glob syntax with separator '/'): ``*`` any run of non-'/' bytes, ``**`` any
run of bytes, ``?`` one non-'/' byte, ``[...]`` / ``[!...]`` a class of bytes and lo-hi ranges
(a '-' that does not stand between two members is a member; a class may hold '/'), ``{a,b}``
alternatives that nest, ``\\c`` the byte c.  ``GlobError`` with ``offset`` for what does not
compile, ``GlobUnsupported`` for extglob, the first from the left deciding."""
import re

import source_oracle as SO

MATCH = 2
GLOB = 5
EXTGLOB = b"!()@+^"
PREFIX_STOP = b"*?[]{}!()@+^"  # globRegex


class GlobError(ValueError):
    def __init__(self, what, offset):
        super().__init__("%s at byte %d" % (what, offset))
        self.offset = offset


class GlobUnsupported(ValueError):
    pass


def _b(s) -> bytes:
    return s if isinstance(s, bytes) else s.encode("utf-8", "surrogateescape")


# ------------------------------------------------------------------ parser and matcher

def parse(glob):
    """The AST: a list of terms ("lit", byte), ("one",), ("star",), ("super",),
    ("class", frozenset of bytes), ("alt", [list of terms, ...])."""
    g = _b(glob)
    at = [0]

    def member():
        if g[at[0]] == 0x5C:
            if at[0] + 1 >= len(g):
                raise GlobError("a trailing backslash", at[0])
            at[0] += 1
        at[0] += 1
        return g[at[0] - 1]

    def klass():
        start = at[0]
        at[0] += 1
        negate = at[0] < len(g) and g[at[0]] == 0x21
        at[0] += negate
        have = set()
        members = 0
        while True:
            if at[0] >= len(g):
                raise GlobError("an unterminated '['", start)
            if g[at[0]] == 0x5D:
                at[0] += 1
                break
            lo_at = at[0]
            lo = hi = member()
            if at[0] + 1 < len(g) and g[at[0]] == 0x2D and g[at[0] + 1] != 0x5D:
                at[0] += 1
                hi = member()
                if hi < lo:
                    raise GlobError("a range whose end is below its start", lo_at)
            have.update(range(lo, hi + 1))
            members += 1
        if not members:
            raise GlobError("an empty class", start)
        return ("class", frozenset(set(range(256)) - have if negate else have))

    def seq(depth):
        out = []
        while at[0] < len(g):
            c = g[at[0]]
            if depth and c in b",}":
                return out
            if c == 0x2A:
                if g[at[0] + 1:at[0] + 2] == b"*":
                    out.append(("super",))
                    at[0] += 2
                else:
                    out.append(("star",))
                    at[0] += 1
            elif c == 0x3F:
                out.append(("one",))
                at[0] += 1
            elif c == 0x5B:
                out.append(klass())
            elif c == 0x7B:
                start = at[0]
                at[0] += 1
                alts = []
                while True:
                    alts.append(seq(depth + 1))
                    if at[0] >= len(g):
                        raise GlobError("an unterminated '{'", start)
                    at[0] += 1
                    if g[at[0] - 1] == 0x7D:
                        break
                out.append(("alt", alts))
            elif c in b"]}":
                raise GlobError("a stray '%c'" % c, at[0])
            elif c in EXTGLOB:
                raise GlobUnsupported("extglob ('%c') at byte %d" % (c, at[0]))
            else:
                out.append(("lit", member()))
        return out

    return seq(0)


def match(ast, s) -> bool:
    """Whether the whole of ``s`` matches: backtracking over the AST with a continuation."""
    s = _b(s)
    n = len(s)

    def run(terms, k, pos, cont):
        if k == len(terms):
            return cont(pos)
        t = terms[k]
        kind = t[0]
        if kind == "lit":
            return pos < n and s[pos] == t[1] and run(terms, k + 1, pos + 1, cont)
        if kind == "one":
            return pos < n and s[pos] != 0x2F and run(terms, k + 1, pos + 1, cont)
        if kind == "class":
            return pos < n and s[pos] in t[1] and run(terms, k + 1, pos + 1, cont)
        if kind == "star":
            end = pos
            while True:
                if run(terms, k + 1, end, cont):
                    return True
                if end >= n or s[end] == 0x2F:
                    return False
                end += 1
        if kind == "super":
            return any(run(terms, k + 1, end, cont) for end in range(pos, n + 1))
        return any(run(alt, 0, pos, lambda p: run(terms, k + 1, p, cont)) for alt in t[1])

    return run(ast, 0, 0, lambda p: p == n)


def positions(ast) -> int:
    """The byte-consuming terms: the positions of the glob's automaton."""
    return sum(sum(positions(a) for a in t[1]) if t[0] == "alt" else 1 for t in ast)


# ------------------------------------------------------------------ translation to re

def to_regex(glob):
    """The glob's text to a bytes regex, term by term (a glob that compiles is assumed)."""
    g = _b(glob)
    out = []
    i, depth = 0, 0

    def esc(b):
        return b"\\x%02x" % b

    while i < len(g):
        c = g[i:i + 1]
        if c == b"*":
            if g[i + 1:i + 2] == b"*":
                out.append(b"(?s:.*)")
                i += 2
            else:
                out.append(b"[^/]*")
                i += 1
        elif c == b"?":
            out.append(b"[^/]")
            i += 1
        elif c == b"[":
            i += 1
            neg = g[i:i + 1] == b"!"
            i += neg
            body = []
            while g[i:i + 1] != b"]":
                def one():
                    nonlocal i
                    if g[i:i + 1] == b"\\":
                        i += 1
                    i += 1
                    return g[i - 1]
                lo = hi = one()
                if g[i:i + 1] == b"-" and g[i + 1:i + 2] not in (b"]", b""):
                    i += 1
                    hi = one()
                body.append(esc(lo) + b"-" + esc(hi))
            i += 1
            out.append(b"[" + (b"^" if neg else b"") + b"".join(body) + b"]")
        elif c == b"{":
            out.append(b"(?:")
            depth += 1
            i += 1
        elif c == b"}" and depth:
            out.append(b")")
            depth -= 1
            i += 1
        elif c == b"," and depth:
            out.append(b"|")
            i += 1
        else:
            if c == b"\\":
                i += 1
            out.append(esc(g[i]))
            i += 1
    return re.compile(b"".join(out), re.S)


def match_regex(glob, s) -> bool:
    return to_regex(glob).fullmatch(_b(s)) is not None


# ------------------------------------------------------------------ the RPCs

def literal_prefix(glob: str) -> str:
    """globLiteralPrefix."""
    g = _b(glob)
    k = min((g.index(bytes([c])) for c in PREFIX_STOP if c in g), default=len(g))
    return g[:k].decode("utf-8", "surrogateescape")


def match_function(arg: str):
    """globMatchFunction(cleanPath(arg))."""
    glob = SO.clean_path(arg)
    ast = parse(glob)

    def mf(path):
        if path == "/" and glob == "/":
            return True
        return match(ast, _b(path).rstrip(b"/"))
    return mf


def stateless_filter(stream, mf):
    """The ``full`` filter for clean paths in ascending order: an item passes iff mf holds for
    it or for one of its proper directory prefixes."""
    out = []
    for path, src in stream:
        pb = _b(path)
        pre = [pb[:k + 1].decode("utf-8", "surrogateescape")
               for k in range(len(pb) - 1) if pb[k] == 0x2F]
        if mf(path) or any(mf(p) for p in pre):
            out.append((path, src))
    return out


def source(entries, arg: str, leaf=None, with_prefix=False, stateless=False):
    """getFile's stream for the glob ``arg``: [(path, tag, src, type, size, hash, flags)] with
    MATCH in the flags of what globFile reports; KeyError where NewErrOnEmpty answers.
    ``with_prefix``: index.WithPrefix(globLiteralPrefix(glob)) applied to the entries first, as
    the reference's open does."""
    mf = match_function(arg)
    keep = list(range(len(entries)))
    if with_prefix:
        pre = _b(literal_prefix(SO.clean_path(arg)))
        keep = [i for i in keep if _b(entries[i][0]).startswith(pre)]
    sub = [entries[i] for i in keep]
    inserted = SO.dir_inserter([e[0] for e in sub])
    stream = stateless_filter(inserted, mf) if stateless else SO.index_filter(inserted, mf, True)
    infos = SO.iterate(stream, sub, [leaf[i] for i in keep] if leaf is not None else None)
    out = [(path, sub[src][1] if src is not None else "", keep[src] if src is not None else None,
            SO.DIR if SO.is_dir(path) else SO.FILE, size, h, MATCH if mf(path) else 0)
           for (path, src), (size, h) in zip(stream, infos)]
    if not out:
        raise KeyError(arg)
    return out


def glob_file(entries, arg: str, leaf=None):
    """globFile: the rows for which mf holds itself; nothing matched is []."""
    try:
        return [r for r in source(entries, arg, leaf) if r[6] & MATCH]
    except KeyError:
        return []


# ------------------------------------------------------------------ random patterns

def random_glob(rng, alphabet="ab./", terms=None, depth=0):
    """A glob that compiles, over ``alphabet``, of 1-6 terms."""
    out = []
    for _ in range(rng.randrange(1, 7) if terms is None else terms):
        r = rng.random()
        if r < 0.45:
            c = rng.choice(alphabet)
            out.append("\\" + c if rng.random() < 0.05 else c)
        elif r < 0.60:
            out.append("*")
        elif r < 0.70:
            out.append("**")
        elif r < 0.78:
            out.append("?")
        elif r < 0.88:
            body = "".join(rng.sample(alphabet, rng.randrange(1, 3)))
            if rng.random() < 0.3:
                body = "a-b" + body
            out.append("[" + ("!" if rng.random() < 0.3 else "") + body + "]")
        elif depth < 2:
            alts = [random_glob(rng, alphabet, rng.randrange(0, 3), depth + 1)
                    for _ in range(rng.randrange(1, 4))]
            out.append("{" + ",".join(alts) + "}")
        else:
            out.append(rng.choice(alphabet))
    return "".join(out)
