"""Seeded generators for the regex-structure tests (CPU and GPU) and the derived pattern that `re` checks the statement against."""
import re

import numpy as np

from repair.regex_structure import ANCHOR_END, ANCHOR_START, Capture, Constant, Program

# ten letters, none a line terminator; the classes are drawn from the alphanumeric ones (a class of the grammar holds nothing else)
ALPHABET = "ab01xy %-9"
CLASS_CHARS = "ab01xy9"


def class_bits(chars):
    bits = 0
    for ch in chars:
        bits |= 1 << ord(ch)
    return bits


def random_program(rng, max_segs=4):
    segs = []
    for _ in range(int(rng.integers(1, max_segs + 1))):
        if rng.random() < 0.35:
            segs.append(Constant("".join(rng.choice(list(ALPHABET), size=int(rng.integers(1, 4))))))
        else:
            chars = rng.choice(list(CLASS_CHARS), size=int(rng.integers(1, 5)), replace=False)
            mn = int(rng.integers(0, 4))
            mx = -1 if rng.random() < 0.2 else mn + int(rng.integers(0, 4))
            segs.append(Capture(class_bits(chars), mn, mx))
    return Program(int(rng.integers(0, 4)), tuple(segs))


def random_string(rng, max_len=12):
    return "".join(rng.choice(list(ALPHABET), size=int(rng.integers(0, max_len + 1))))


def random_cases(n, seed=20240611, per_program=1):
    """n (program, string) pairs, `per_program` strings in a row to one program."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        program = random_program(rng)
        out.extend((program, random_string(rng)) for _ in range(per_program))
    return out[:n]


def pooled_cases():
    """The 5 000 cases both suites run: eight strings to a program, so that a device call sees a pool (the CPU suite holds them to `re`)."""
    return random_cases(5000, seed=20240612, per_program=8)


def derived_regex(program):
    """The regex `RegexStructureRepair` derives from a program, in the syntax Python's `re` shares with java.util.regex for this
    sub-language; a wildcard is spelled as the complement of Java's line terminators, `$` as the true end."""
    parts = ["^"] if program.anchors & ANCHOR_START else []
    for seg in program.segs:
        if isinstance(seg, Constant):
            parts.append("[^\\n\\r\\x85\\u2028\\u2029]{1,%d}" % len(seg.text))
        else:
            chars = "".join("\\x%02x" % c for c in range(128) if (seg.cls >> c) & 1)
            parts.append("([%s]{%d,%s})" % (chars, seg.min, "" if seg.max < 0 else seg.max))
    if program.anchors & ANCHOR_END:
        parts.append("\\Z")
    return "".join(parts)


def re_repair(program, s):
    """What `RegexStructureRepair.apply` computes, by `re.search` on the derived pattern: the captures and the literal constants in order."""
    m = re.search(derived_regex(program), s)
    if m is None:
        return None
    out, g = [], 1
    for seg in program.segs:
        if isinstance(seg, Constant):
            out.append(seg.text)
        else:
            out.append(m.group(g))
            g += 1
    return "".join(out)


__all__ = ["ALPHABET", "ANCHOR_END", "ANCHOR_START", "class_bits", "random_program", "random_string", "random_cases", "pooled_cases", "re_repair"]
