"""How the fixtures of recorded calls (tests/golden/abi_error_paths.json, consumer_call_errors.json) hold the pairs of faults.

A row is [name, changes, *outcome].  The rows of one name stand together: the call without a fault, one row per single
fault, then [name, "pairs", lines] and the rows of the pairs that row marks "?".  lines[i][j - i - 1] says what the call
with fault i and fault j (i < j, counted in the order of the single-fault rows) gave: "a" the outcome of fault i alone, "b"
that of fault j alone - which is what pins the order of the checks -, "?" another one, written out in a row of its own, and
"-" that the pair is not made because both faults change the same argument.  `pack` writes this form and `unpack` gives
back one row per call; names without a "pairs" row pass through as they are."""


def pair_changes(faults):
    """(i, j, merged changes or None) for every i < j; None where the two faults change the same argument."""
    return [(i, j, None if set(faults[i]) & set(faults[j]) else {**faults[i], **faults[j]})
            for i in range(len(faults)) for j in range(i + 1, len(faults))]


def pack(name, head, faults, run):
    """The rows of `name`: `run(changes)` -> outcome (a list) for the call `head`, every fault and every pair."""
    single = [run(m) for m in faults]
    lines, extra = [""] * max(len(faults) - 1, 0), []
    for i, j, both in pair_changes(faults):
        got = None if both is None else run(both)
        mark = "-" if both is None else "a" if got == single[i] else "b" if got == single[j] else "?"
        lines[i] += mark
        if mark == "?":
            extra.append([name, both, *got])
    return [[name, head, *run(head)]] + [[name, m, *o] for m, o in zip(faults, single)] + [[name, "pairs", lines]] + extra


def unpack(rows):
    """One row per call, in the order head, single faults, pairs."""
    out, k = [], 0
    while k < len(rows):
        name, block = rows[k][0], []
        while k < len(rows) and rows[k][0] == name:
            block.append(rows[k])
            k += 1
        at = [n for n, r in enumerate(block) if r[1] == "pairs"]
        if not at:
            out += block
            continue
        plain, lines, extra = block[:at[0]], block[at[0]][2], block[at[0] + 1:]
        faults, single = [r[1] for r in plain[1:]], [r[2:] for r in plain[1:]]
        out += plain
        for i, j, both in pair_changes(faults):
            mark = lines[i][j - i - 1]
            assert (mark == "-") == (both is None), (name, i, j)
            if mark == "?":
                out.append(next(r for r in extra if r[1] == both))
            elif mark != "-":
                out.append([name, both, *single[i if mark == "a" else j]])
    return out
