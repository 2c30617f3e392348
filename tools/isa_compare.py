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


_PCREL = re.compile(r"^s_add_u32 (s\d+|vcc_lo), \1, (0x[0-9a-f]+)$")      # (the register allocator also hands the pair's low half to vcc_lo)


def address_shift(x, y):
    """What the differing instructions of one symbol are.  A kernel added to (or taken from) the library adds its 64-byte descriptor to
    .rodata, which lies between the constant tables and .text: every pc-relative address of a table (s_getpc_b64; s_add_u32 sN, sN,
    <literal>; s_addc_u32) then moves by that much and nothing else does.  -> (differing instructions, the set of literal shifts if every
    one of them is such an s_add_u32 on both sides, else None)"""
    if len(x) != len(y):
        return abs(len(x) - len(y)) + sum(p != q for p, q in zip(x, y)), None
    shifts, n = set(), 0
    for p, q in zip(x, y):
        if p == q:
            continue
        n += 1
        mp, mq = _PCREL.match(p), _PCREL.match(q)
        if not (mp and mq and mp.group(1) == mq.group(1)):
            return sum(s != t for s, t in zip(x, y)), None
        shifts.add((int(mq.group(2), 16) - int(mp.group(2), 16)) & 0xffffffff)
    return n, shifts


def main():
    a, b = symbols(sys.argv[1]), symbols(sys.argv[2])
    differing = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    res = {"symbols_before": len(a), "symbols_after": len(b), "only_before": sorted(set(a) - set(b)), "only_after": sorted(set(b) - set(a)),
           "compared": len(set(a) & set(b)), "instructions_compared": sum(len(a[k]) for k in set(a) & set(b)),
           "differing": len(differing), "differing_symbols": differing}
    # of the differing symbols: those whose every differing instruction is the literal of a pc-relative table address, and the others
    kinds = {k: address_shift(a[k], b[k]) for k in differing}
    res["differing_instructions"] = sum(n for n, _ in kinds.values())
    res["differing_other_than_table_addresses"] = sorted(k for k, (_, s) in kinds.items() if s is None)
    res["table_address_shifts_bytes"] = sorted(set().union(*[s for _, s in kinds.values() if s]))
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text + "\n")
    return 1 if (differing or res["only_before"] or res["only_after"]) else 0


if __name__ == "__main__":
    sys.exit(main())
