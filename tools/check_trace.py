#!/usr/bin/env python3
"""tools/check_trace.py <pie> [settings]: which rows and which logup tuples break a trace (`lmn_trace_check`).

`lmn_prove` answers a bad trace with ProverError(ConstraintsNotSatisfied) at the end of a whole proof, and proves a trace
whose relations do not balance all the same (only the verifier says InvalidLogUp).  This prints, for the same input: the
local constraint slots that are non-zero on real rows (table, slot, how many rows, the first), the logup tuples whose net
multiplicity is not zero (element set, value, tensor id, net, first mention) and the words that are no canonical M31.

<pie>       an .npz file with one array per trace table, named kind_<K> (K = LMN_KIND_*, TraceTable variant order): the rows,
            n_rows x n_columns(K) uint32 words in `Column::index()` order - `numpy.savez(path, kind_0=add_rows, kind_1=...)`
[settings]  CircuitSettings as bincode or JSON (luminair_amd.pie.CircuitSettings), needed when the pie has lookup tables

Exit status: 0 the trace is clean, 1 something was found, 2 the input was refused (the text names the table)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from luminair_amd import backend                                   # noqa: E402
from luminair_amd.pie import CircuitSettings, TraceTableKind       # noqa: E402


def load_pie(path):
    data = np.load(path)
    tables = []
    for name in data.files:
        if not name.startswith("kind_"):
            raise SystemExit("%s: array %r is not named kind_<K>" % (path, name))
        tables.append((int(name[5:]), np.ascontiguousarray(data[name], dtype=np.uint32)))
    return sorted(tables, key=lambda kt: kt[0])


def load_settings(path):
    raw = open(path, "rb").read()
    return CircuitSettings.from_json(raw.decode()) if raw.lstrip()[:1] == b"{" else CircuitSettings.from_bincode(raw)


def kind_name(kind):
    try:
        return TraceTableKind(kind).name
    except ValueError:
        return "kind %d" % kind


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pie")
    ap.add_argument("settings", nargs="?")
    ap.add_argument("--variant", choices=("kat", "pinned"), default="pinned", help="protocol variant (decides which kinds have a claim slot)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--library", help="path of the backend library (default: the package's libluminair_hip.so)")
    args = ap.parse_args()
    lib = backend.Library(args.library)
    cfg = lib.default_config()
    cfg.protocol_variant = backend.VARIANT_PINNED if args.variant == "pinned" else backend.VARIANT_KAT
    ctx = backend.Context(args.device, cfg, lib)
    tables = load_pie(args.pie)
    luts = load_settings(args.settings).lut_columns(lib) if args.settings else None
    try:
        rep = ctx.check_trace([(k, r, len(r)) for k, r in tables], luts)
    except backend.LuminairBackendError as e:
        print("refused: %s" % e)
        return 2
    finally:
        ctx.close()
    print(rep.summary)
    for i, (k, r) in enumerate(tables):
        print("table %d: %s, %d rows" % (i, kind_name(k), len(r)))
    if rep.n_noncanonical:
        t, r, c = rep.first_noncanonical
        print("non-canonical words: %d, first at table %d row %d column %d (rows holding one are left out below)"
              % (rep.n_noncanonical, t, r, c))
    if rep.n_constraint_slots:
        print("violated constraint slots: %d%s" % (rep.n_constraint_slots, " (first %d listed)" % len(rep.constraints)
                                                   if rep.constraints_truncated else ""))
        for t, k, slot, count, first in rep.constraints:
            print("  table %d (%s) slot %d: %d rows, first row %d" % (t, kind_name(k), slot, count, first))
    if rep.n_unbalanced:
        print("unbalanced tuples: %d%s" % (rep.n_unbalanced, " (%d of them listed)" % len(rep.tuples) if rep.tuples_truncated else ""))
        for s, val, ident, net, ft, fs, fr in rep.tuples:
            signed = net - backend_P if net > backend_P // 2 else net
            print("  %s id %d val %d: net %d, first mentioned by table %d slot %d row %d"
                  % (backend.ELEM_SET_NAMES[s], ident, val, signed, ft, fs, fr))
    return 0 if rep.ok else 1


backend_P = (1 << 31) - 1   # M31

if __name__ == "__main__":
    sys.exit(main())
