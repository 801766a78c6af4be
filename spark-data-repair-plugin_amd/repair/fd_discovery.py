"""Level-wise discovery of the minimal (approximate) functional dependencies of a table from the integers of `fd_measures` alone
(`Table.fd_measures` on the resident table, `repair.fd_codes.fd_measures` without a device): DESIGN.md 5o.  The search reads nothing but
those integers and compares them exactly, so both paths give the same list."""
import itertools
from fractions import Fraction
from typing import Any, Callable, Dict, List, Optional, Sequence

MAX_LHS_SIZE = 4


def max_removed_rows(max_error: str, n: int) -> int:
    """floor(max_error * n), taken exactly from the option's decimal text (0.29 * 100 is 29, where floating point says 28.999...)."""
    return int(Fraction(str(max_error).strip()) * n)          # (int() of a non-negative Fraction is its floor)


def discover(measure: Callable[[List[int], List[int]], Dict[str, Any]], n: int, columns: Sequence[str], targets: Sequence[str],
             max_lhs_size: int = 2, max_error: str = "0.0", max_lhs_group_ratio: str = "1.0", log: Optional[List[str]] = None,
             stats: Optional[Dict[str, int]] = None, prune_equal_partitions: bool = True) -> List[Dict[str, Any]]:
    """The dependencies X -> Y, |X| <= `max_lhs_size` (1 .. 4), Y in `targets`, that hold after removing at most floor(max_error * n) of
    the `n` rows and have no proper subset of X that does.  `columns`: the names of the table's columns, by position (the position is what
    `measure(lhs, rhs_cols)` takes); `targets`: those allowed as a right-hand side.

      level 0   one call with X = {}: a column that holds under {} is constant within the threshold; it leaves both sides (`log` hears of it)
      level k   X over the k-subsets of the remaining columns in column order, one call per X, skipped when a subset of X is a key
                (groups == n) or has more than max_lhs_group_ratio * n groups, when X holds X' and A of a recorded exact X' -> A (the same
                partition as X without A), or when no right-hand side is left: the targets outside X that no proper subset of X determines.
                The results of an X that is itself a key are discarded.

    Records dict(lhs = names in column order, rhs, groups, removed_rows, violating_rows, xy_groups), ordered by |X|, the positions of X, the
    position of Y.  `stats`, when given, receives `calls` (measure calls made) and `skipped` (left-hand sides not measured)."""
    if not 1 <= int(max_lhs_size) <= MAX_LHS_SIZE:
        raise ValueError("max_lhs_size must be in [1, %d]" % MAX_LHS_SIZE)
    names = list(columns)
    pos = {c: j for j, c in enumerate(names)}
    if any(t not in pos for t in targets):
        raise ValueError("a target is not among the columns")
    limit = max_removed_rows(max_error, n)
    ratio = Fraction(str(max_lhs_group_ratio).strip())
    if limit < 0 or ratio < 0:
        raise ValueError("max_error and max_lhs_group_ratio must not be negative")
    calls = skipped = 0
    records: List[Dict[str, Any]] = []
    if n > 0 and names:
        every = list(range(len(names)))
        m = measure([], every)
        calls += 1
        constant = {j for j in every if n - int(m["kept"][j]) <= limit}
        if constant and log is not None:
            log.append("constant within the threshold, on neither side: %s" % ", ".join(names[j] for j in sorted(constant)))
        live = [j for j in every if j not in constant]
        rhs_all = [pos[t] for t in names if t in set(targets) and pos[t] not in constant]
        blocked: List[frozenset] = []                       # keys and left-hand sides of too many groups: no superset is looked at
        same: List[frozenset] = []                          # X' + {A} of every recorded exact X' -> A
        holds: Dict[int, List[frozenset]] = {y: [] for y in rhs_all}
        for k in range(1, int(max_lhs_size) + 1):
            for X in itertools.combinations(live, k):
                xs = frozenset(X)
                rhs = [y for y in rhs_all if y not in xs and not any(h < xs for h in holds[y])]
                if any(b <= xs for b in blocked) or (prune_equal_partitions and any(e <= xs for e in same)) or not rhs:
                    skipped += 1
                    continue
                m = measure(list(X), rhs)
                calls += 1
                groups = int(m["groups"])
                if groups == n or groups > ratio * n:
                    blocked.append(xs)
                if groups == n:
                    continue
                for r, y in enumerate(rhs):
                    removed = n - int(m["kept"][r])
                    if removed > limit:
                        continue
                    holds[y].append(xs)
                    if removed == 0:
                        same.append(xs | {y})
                    records.append(dict(lhs=[names[j] for j in X], rhs=names[y], groups=groups, removed_rows=removed,
                                        violating_rows=int(m["violating"][r]), xy_groups=int(m["xy_groups"][r])))
    if stats is not None:
        stats["calls"], stats["skipped"] = calls, skipped
    return records
