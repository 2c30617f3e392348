#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libedcore.so, symbol by symbol: for a change that must not touch any kernel.

The code object is taken out of each library and disassembled as tools/isa_hazard_scan.py does; of every line only the instruction
text is kept (addresses and encodings, which move with a symbol's place in the object, are dropped).  Text only: nothing is looked
for in it.

    python tools/isa_compare.py BEFORE.so AFTER.so [out.json]      exit status 1 if a symbol differs or exists on one side only
"""
import json
import re
import sys

from isa_hazard_scan import disassemble, extract_code_object


def symbols(so_path):
    """-> {symbol: [instruction text, ...]}"""
    out = {}
    cur = None
    for line in disassemble(extract_code_object(so_path)).split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        t = line.split("//")[0].strip()
        if t and cur is not None:
            cur.append(t)
    return out


def main():
    a, b = symbols(sys.argv[1]), symbols(sys.argv[2])
    differing = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    res = {"symbols_before": len(a), "symbols_after": len(b), "only_before": sorted(set(a) - set(b)), "only_after": sorted(set(b) - set(a)),
           "compared": len(set(a) & set(b)), "instructions_compared": sum(len(a[k]) for k in set(a) & set(b)),
           "differing": len(differing), "differing_symbols": differing}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text + "\n")
    return 1 if (differing or res["only_before"] or res["only_after"]) else 0


if __name__ == "__main__":
    sys.exit(main())
