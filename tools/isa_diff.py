#!/usr/bin/env python3
"""Are the kernels of two device listings of one translation unit (csrc/sgo_conv.hip, sgo_engine.hip, sgo_rules.hip) the same
machine code?  The check behind a source-only change: the tower kernels (csrc/sgo_conv_tile.hpp: shared pieces are macros so
that this holds), the engine's split into sgo_engine_state.hpp / sgo_search.hpp / sgo_engine_inspect.hpp, the board_advance
preamble of sgo_rules.hip.  Per kernel symbol: the text from its label to .end_amdhsa_kernel with `;` comments removed, and
VGPRs / LDS bytes / scratch bytes from its descriptor.  Local labels carry the ordinal of their function in the file (.LBB64_2);
it is dropped, so that removing an instantiation does not make every later kernel look different.

usage: isa_diff.py OLD.s NEW.s [symbol prefix ...]     (listings: vmcnt_isa_check.device_asm(source="sgo_engine.hip"), or
       hipcc --cuda-device-only -S with the flags of sejonggo_amd/build.py, run inside a sejonggo_amd/csrc-shaped tree because
       sgo_common.hpp includes ../../include/sgo.h; add -DSGO_CONV4W_VARIANTS for the conv's selectable schedule variants)
Without prefixes every kernel of OLD is compared; a kernel missing from NEW is reported and is no failure (retired variants).
Exit status 1 if a kernel present in both differs."""
import re
import sys


def kernels(asm):
    return re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)


def body(asm, sym):
    lines = asm.split("\n")
    i = next(j for j, l in enumerate(lines) if l.startswith(sym + ":"))
    k = lines[i:next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])]
    return [re.sub(r"(\.L[A-Za-z_]+?)\d+(_\d+)?\b", r"\1\2", l.split(";")[0].rstrip()) for l in k if l.split(";")[0].strip()]


def meta(text, key):
    return next((l.split()[-1] for l in text if l.strip().startswith(key)), "?")


def main():
    old, new = open(sys.argv[1]).read(), open(sys.argv[2]).read()
    want = sys.argv[3:]
    rc = 0
    for sym in kernels(old):
        if want and not any(sym.startswith(w) for w in want):
            continue
        if sym not in kernels(new):
            print("%-60s only in %s" % (sym, sys.argv[1]))
            continue
        a, b = body(old, sym), body(new, sym)
        m = ["%s/%s/%s" % tuple(meta(t, k) for k in (".amdhsa_next_free_vgpr", ".amdhsa_group_segment_fixed_size", ".amdhsa_private_segment_fixed_size"))
             for t in (a, b)]
        same = a == b
        print("%-60s lines %5d %5d  vgpr/lds/scratch %s %s  %s" % (sym, len(a), len(b), m[0], m[1], "EQUAL" if same else "DIFFERENT"))
        rc |= not same
    for sym in kernels(new):
        if sym not in kernels(old) and (not want or any(sym.startswith(w) for w in want)):
            print("%-60s only in %s" % (sym, sys.argv[2]))
    sys.exit(rc)


if __name__ == "__main__":
    main()
