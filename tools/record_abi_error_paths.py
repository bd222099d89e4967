#!/usr/bin/env python3
"""Record the consumer rows of tests/golden/abi_error_paths.json from a given build.

    python tools/record_abi_error_paths.py [--build ROOT] [--out FILE]

ROOT is the checkout whose deepmimo_amd package and built library answer the calls (default: this one) - to pin today's
behaviour ahead of a change of deepmimo_amd/csrc/dmx_abi.hip, a built checkout of the commit before it.  The calls are
`_abi_consumer_faults()` of tests/test_host_cpu.py - singles and pairs, packed by tests/_pair_rows.py - made by its
`_abi_call`; the rows of the other entry points are carried
over from the existing file as they are.  Needs no GPU and must never reach a launch: a row that comes back DMX_ERR_LAUNCH,
or with rc 0 from a launching entry point that was given users, stops the recording.
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
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "abi_error_paths.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.build))
    from deepmimo_amd import _native as n
    assert os.path.abspath(n.__file__).startswith(os.path.abspath(args.build) + os.sep), n.__file__
    sys.path.insert(0, HERE)                                      # tests/ of this checkout, whatever the build holds
    spec = importlib.util.spec_from_file_location("_host_cpu_tests", os.path.join(HERE, "tests", "test_host_cpu.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    from tests._pair_rows import pack
    lib = n.load()
    faults = t._abi_consumer_faults()
    rows = [r for r in json.load(open(args.out)) if r[0] not in faults]

    def run(entry, mods):
        rc, msg = t._abi_call(lib, n, entry, mods)
        if rc == -3:
            sys.exit(f"{entry} {mods}: DMX_ERR_LAUNCH ({msg}) - the call got past the validation")
        if not entry.endswith("_ok") and (rc > 0 or (rc == 0 and mods.get("count") != 0)):
            sys.exit(f"{entry} {mods}: rc {rc} - a launching entry point accepted a call that has users")
        return [rc, msg if rc < 0 or (rc == 0 and entry.endswith("_ok")) else ""]
    for entry, fs in faults.items():
        rows += pack(entry, t._abi_consumer_head(entry), fs, lambda mods, entry=entry: run(entry, mods))
    with open(args.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows (the consumers' recorded from {n.LIB_PATH}) -> {args.out}")


if __name__ == "__main__":
    main()
