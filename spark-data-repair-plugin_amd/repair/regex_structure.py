"""Regex-structure repair in value space: the statement of `RegexStructureRepair.scala` (reference
src/main/scala/org/apache/spark/python/RegexStructureRepair.scala, grammar src/main/antlr4/.../RegexBase.g4,
`RepairApi.repairByRegularExpression`, RepairApi.scala:677-704).  Host code only; `rgbm_regex_structure` (csrc/rgbm_regex.hip) is held to
it integer for integer.

A regex such as `^[0-9]{1,3} patients$` is reduced to a STRUCTURE: the counted character-class runs (`[0-9]{1,3}`, lexer rule RANGE) are
captured, the constants (` patients`, rule CONSTANT) are matched loosely as `.{1,len}`, `^` first and `$` last are kept, and everything
else (a class without a count, `.`, `*`, `+`, `?`, `|`) vanishes -- the reference's "naive approach".  A dirty value that the derived regex
finds (`findFirstMatchIn`) is rewritten from its captures and the literal constants: `32 patixxts` -> `32 patients`.

`parse` restates the ANTLR lexer (longest match, ties to the earliest rule, in the order PATTERN, SYMBOL, RANGE, CONSTANT, STAR, PLUS,
MAYBE, ALTERNATION, ANY, CARET, DOLLAR, CHARACTER, NUMBER; WS = tab, CR, LF is skipped) and the grammar `CARET? expression DOLLAR?`,
flattened as `RegexRewriteVisiter` does.  Refused (`NotRepairable`, which the callers log and turn into "no repair from this detector", the
outcome the reference reaches through the exception `repairByRegularExpression` catches):
  * a character the lexer has no rule for;
  * a token sequence the grammar does not consume to its end (a lone letter or digit lexes as SYMBOL, which no parser rule takes: `f[0-9]`);
  * a class range written backwards (`[z-a]`), `{m,n}` with m > n (java.util.regex refuses both);
  * the `{,n}` form: java.util.regex rejects it as far as is known; Java cannot be run where this was written, so this is stated, not checked;
  * a bound above 65 535, more than 32 segments (the device program's limits);
  * a program without a segment: it would turn every cell into the empty string.
The reference's parser has no error listener and no EOF in its start rule, so what IT does with a token sequence that the grammar does not
consume depends on ANTLR's error recovery, which could not be run either: refusing those sequences is the one place where this statement is
deliberately narrower than the reference may be.

Matching (`repair_value`) means `findFirstMatchIn` on the derived regex: leftmost start, every segment greedy, the first successful
backtracking path.  It is stated without backtracking: F[i] = the positions from which segments i.. can finish (F[S] = {len} with `$`, every
position without), built backwards; the start is the least position of F[0] (0 with `^`); forwards every segment takes the largest count
k in [min, min(max, run length)] with p + k in F[i + 1].

A wildcard (a constant's `.`) matches any code point except U+000A, U+000D, U+0085, U+2028, U+2029 (Java's `.`), `$` is the true end of
the string.  Java's and Python's `$` differ next to a final line terminator and neither could be checked, so the CALLERS leave a value
that holds one of these five code points to the models (`has_line_terminator`)."""
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

MAX_SEGS = 32
MAX_BOUND = 65535
ANCHOR_START, ANCHOR_END = 1, 2
LINE_TERMINATORS = frozenset((0x0A, 0x0D, 0x85, 0x2028, 0x2029))

_LETTERS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
_DIGITS = "0123456789"
_ALNUM = frozenset(_LETTERS + _DIGITS)
_CONST = frozenset(_LETTERS + _DIGITS + " _-%")
_WS = frozenset("\t\r\n")
_SINGLE = {"*": "STAR", "+": "PLUS", "?": "MAYBE", "|": "ALTERNATION", ".": "ANY", "^": "CARET", "$": "DOLLAR"}
_RULE_ORDER = ["PATTERN", "SYMBOL", "RANGE", "CONSTANT", "STAR", "PLUS", "MAYBE", "ALTERNATION", "ANY", "CARET", "DOLLAR", "CHARACTER", "NUMBER"]


class NotRepairable(ValueError):
    """The pattern gives no structure to repair with; str(e) is the reason."""


class Capture(NamedTuple):
    cls: int                  # bit c = ASCII code point c is in the class (128 bits)
    min: int
    max: int                  # -1: unbounded


class Constant(NamedTuple):
    text: str                 # matched as a wildcard run of 1 .. len(text) code points, written back literally


class Program(NamedTuple):
    anchors: int              # bit 0: `^`, bit 1: `$`
    segs: Tuple[Union[Capture, Constant], ...]


def _match_pattern(s: str, i: int) -> int:
    """Length of PATTERN at s[i:] ('[' (CHARACTER | CHARACTER '-' CHARACTER)+ ']'), 0: none."""
    if i >= len(s) or s[i] != "[":
        return 0
    j, items = i + 1, 0
    while j < len(s) and s[j] in _ALNUM:
        j += 3 if j + 2 < len(s) and s[j + 1] == "-" and s[j + 2] in _ALNUM else 1
        items += 1
    return j + 1 - i if items and j < len(s) and s[j] == "]" else 0


def _match_number(s: str, i: int) -> int:
    j = i
    while j < len(s) and s[j] in _DIGITS:
        j += 1
    return j - i


def _match_range(s: str, i: int, symbol: int) -> int:
    """Length of RANGE at s[i:] given the length of its SYMBOL, 0: none.  One SYMBOL fits a position at most (a letter or a class)."""
    j = i + symbol
    if not symbol or j >= len(s) or s[j] != "{":
        return 0
    j += 1
    a = _match_number(s, j)
    j += a
    if j < len(s) and s[j] == ",":
        j += 1
        b = _match_number(s, j)
        j += b
        if not a and not b:
            return 0
    elif not a:
        return 0
    return j + 1 - i if j < len(s) and s[j] == "}" else 0


def tokenize(pattern: str) -> List[Tuple[str, str]]:
    """The (rule, text) tokens of RegexBase.g4's lexer; raises NotRepairable at a character without a rule."""
    out: List[Tuple[str, str]] = []
    i = 0
    while i < len(pattern):
        ch = pattern[i]
        if ch in _WS:
            i += 1
            continue
        cand: Dict[str, int] = {}
        cand["PATTERN"] = _match_pattern(pattern, i)
        cand["SYMBOL"] = cand["PATTERN"] or (1 if ch in _ALNUM else 0)
        cand["RANGE"] = _match_range(pattern, i, cand["SYMBOL"])
        j = i
        while j < len(pattern) and pattern[j] in _CONST:
            j += 1
        cand["CONSTANT"] = j - i
        if ch in _SINGLE:
            cand[_SINGLE[ch]] = 1
        cand["CHARACTER"] = 1 if ch in _ALNUM else 0
        cand["NUMBER"] = _match_number(pattern, i)
        best = max(cand.values())
        if best == 0:
            raise NotRepairable("the lexer has no rule for %r at position %d" % (ch, i))
        rule = next(r for r in _RULE_ORDER if cand.get(r, 0) == best)      # ties: the earliest rule
        out.append((rule, pattern[i:i + best]))
        i += best
    return out


_ATOMS = ("CONSTANT", "ANY", "PATTERN", "RANGE")
_POSTFIX = ("STAR", "PLUS", "MAYBE")


def flatten(pattern: str) -> List[Tuple[str, str]]:
    """`RegexParser.parse`: the (Other | Pattern | Constant, text) sequence of a pattern the grammar consumes to its end."""
    toks = tokenize(pattern)
    body = list(toks)
    out: List[Tuple[str, str]] = []
    tail: List[Tuple[str, str]] = []
    if body and body[0][0] == "CARET":
        out.append(("Other", body.pop(0)[1]))
    if body and body[-1][0] == "DOLLAR":
        tail.append(("Other", body.pop()[1]))
    # expression: atom | e postfix | e e | e '|' e  ==  an atom first, an atom after every '|', no '|' last
    if not body:
        raise NotRepairable("the grammar needs an expression")
    prev = None
    for rule, text in body:
        if rule in _ATOMS:
            pass
        elif rule in _POSTFIX or rule == "ALTERNATION":
            if prev is None or prev == "ALTERNATION":
                raise NotRepairable("the grammar does not take %s `%s` here" % (rule, text))
        else:
            raise NotRepairable("the grammar does not take %s `%s`%s" % (
                rule, text, " (a lone letter or digit is a SYMBOL, not a CONSTANT)" if rule == "SYMBOL" else ""))
        prev = rule
        if rule == "CONSTANT":
            out.append(("Constant", text))
        elif rule == "RANGE":
            out.append(("Pattern", text))
    if prev == "ALTERNATION":
        raise NotRepairable("the grammar does not take ALTERNATION `|` last")
    return out + tail


def _capture(text: str) -> Capture:
    brace = text.index("{")
    sym, count = text[:brace], text[brace + 1:-1]
    cls = 0
    if sym[0] == "[":
        j = 1
        while sym[j] != "]":
            if sym[j + 1] == "-":
                lo, hi = ord(sym[j]), ord(sym[j + 2])
                if lo > hi:
                    raise NotRepairable("the class range `%s` is written backwards" % sym[j:j + 3])
                for c in range(lo, hi + 1):
                    cls |= 1 << c
                j += 3
            else:
                cls |= 1 << ord(sym[j])
                j += 1
    else:
        cls = 1 << ord(sym)
    if "," in count:
        a, b = count.split(",")
        if not a:
            raise NotRepairable("the `{,n}` form of `%s` (java.util.regex rejects it)" % text)
        mn, mx = int(a), (int(b) if b else -1)
    else:
        mn = mx = int(count)
    if mn > MAX_BOUND or mx > MAX_BOUND:
        raise NotRepairable("a bound of `%s` is above %d" % (text, MAX_BOUND))
    if mx >= 0 and mn > mx:
        raise NotRepairable("`%s` has min > max" % text)
    return Capture(cls, mn, mx)


def parse(pattern: str) -> Program:
    """The program of a pattern, or NotRepairable(reason)."""
    anchors = 0
    segs: List[Union[Capture, Constant]] = []
    for kind, text in flatten(pattern):
        if kind == "Other":
            anchors |= ANCHOR_START if text == "^" else ANCHOR_END
        elif kind == "Constant":
            segs.append(Constant(text))
        else:
            segs.append(_capture(text))
    if not segs:
        raise NotRepairable("no counted class and no constant: every value would become the empty string")
    if len(segs) > MAX_SEGS:
        raise NotRepairable("%d segments, more than %d" % (len(segs), MAX_SEGS))
    return Program(anchors, tuple(segs))


def has_line_terminator(s: str) -> bool:
    return any(ord(ch) in LINE_TERMINATORS for ch in s)


def _bounds(seg: Union[Capture, Constant]) -> Tuple[int, int]:
    return (1, len(seg.text)) if isinstance(seg, Constant) else (seg.min, seg.max)


def _member(seg: Union[Capture, Constant], ch: str) -> bool:
    c = ord(ch)
    if isinstance(seg, Constant):
        return c not in LINE_TERMINATORS
    return c < 128 and bool((seg.cls >> c) & 1)


def repair_value(program: Program, s: Optional[str]) -> Optional[str]:
    """The repaired string, or None when the structure is not found in `s` (or `s` is None)."""
    if s is None:
        return None
    n, S = len(s), len(program.segs)
    # prev[q] = the largest position <= q of F[i + 1], -1: none (q in 0 .. n)
    if program.anchors & ANCHOR_END:
        prev = [-1] * n + [n]
    else:
        prev = list(range(n + 1))
    prevs: List[List[int]] = [prev]
    for seg in reversed(program.segs):
        mn, mx = _bounds(seg)
        nxt = prevs[-1]
        f = [False] * (n + 1)
        run = 0                                               # members from p on
        for p in range(n, -1, -1):
            run = run + 1 if p < n and _member(seg, s[p]) else 0
            hi = run if mx < 0 or mx > run else mx
            f[p] = mn <= hi and nxt[p + hi] >= p + mn
        cur, last = [], -1
        for p in range(n + 1):
            if f[p]:
                last = p
            cur.append(last)
        prevs.append(cur)
    prevs.reverse()                                           # prevs[i] describes F[i]
    f0 = prevs[0]
    if f0[n] < 0:
        return None
    p = next(q for q in range(n + 1) if f0[q] == q)           # the least position of F[0]
    if (program.anchors & ANCHOR_START) and p != 0:
        return None
    out: List[str] = []
    for i, seg in enumerate(program.segs):
        mn, mx = _bounds(seg)
        run = 0
        while p + run < n and _member(seg, s[p + run]) and (mx < 0 or run < mx):
            run += 1
        q = prevs[i + 1][p + run]                             # greedy: the largest count that lets the rest finish
        assert q >= p + mn
        out.append(seg.text if isinstance(seg, Constant) else s[p:q])
        p = q
    return "".join(out)


def repair_values(program: Program, strings: Sequence[Optional[str]]) -> List[Optional[str]]:
    """`repair_value` over a pool: what a CPU engine uses as `regex_structure`."""
    return [repair_value(program, s) for s in strings]


def repair_cells(program: Program, strings: Sequence[Optional[str]], evaluate: Any = repair_values) -> Tuple[List[Optional[str]], int]:
    """What both callers (the value-space path of `RepairModel` and the resident pipeline) do with the current values of an attribute's
    error cells: every DISTINCT string is evaluated once (`evaluate(program, strings)`: the statement, or an engine's `regex_structure`);
    None is not repaired, and a value that holds a line terminator is left to the models.  Returns the repaired string or None per
    cell and the number of cells left alone for a terminator."""
    pool = list(dict.fromkeys(s for s in strings if s is not None and not has_line_terminator(s)))
    by_value = dict(zip(pool, evaluate(program, pool))) if pool else {}
    skipped = sum(1 for s in strings if s is not None and s not in by_value)
    return [None if s is None else by_value.get(s) for s in strings], skipped


def program_arrays(program: Program) -> Dict[str, Any]:
    """The program as `rgbm_regex_structure` takes it: per segment (kind, min, max, cls[4], const_off, const_len) and the constants' code points."""
    rows, const_cp = [], []
    for seg in program.segs:
        if isinstance(seg, Constant):
            rows.append((1, 1, len(seg.text), (0, 0, 0, 0), len(const_cp), len(seg.text)))
            const_cp.extend(ord(ch) for ch in seg.text)
        else:
            rows.append((0, seg.min, seg.max, tuple((seg.cls >> (32 * w)) & 0xFFFFFFFF for w in range(4)), 0, 0))
    return dict(segs=rows, const_cp=const_cp, anchors=program.anchors)
