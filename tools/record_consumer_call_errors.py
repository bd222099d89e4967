#!/usr/bin/env python3
"""Record tests/golden/consumer_call_errors.json from a given build.

    python tools/record_consumer_call_errors.py [--build ROOT] [--out FILE]

ROOT is the checkout whose deepmimo_amd package and built library answer the calls (default: this one) - to pin today's
behaviour ahead of a change of the host checks, a built checkout of the commit before it.  The calls and the way an outcome is
written down are those of tests/test_consumer_call_errors_cpu.py (`_faults`, `outcome`; pairs packed by tests/_pair_rows.py).  Needs no GPU.
"""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--build", default=HERE)
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "consumer_call_errors.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.build))
    import deepmimo_amd
    assert os.path.abspath(deepmimo_amd.__file__).startswith(os.path.abspath(args.build) + os.sep), deepmimo_amd.__file__
    sys.path.insert(0, HERE)                                      # tests/ and the oracle of this checkout
    spec = importlib.util.spec_from_file_location("_consumer_call_tests", os.path.join(HERE, "tests", "test_consumer_call_errors_cpu.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    from tests._pair_rows import pack
    rows = [r for name, faults in t._faults().items() for r in pack(name, {}, faults, lambda ch, name=name: t.outcome(name, ch))]
    with open(args.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows recorded from {os.path.dirname(deepmimo_amd.__file__)} -> {args.out}")


if __name__ == "__main__":
    main()
