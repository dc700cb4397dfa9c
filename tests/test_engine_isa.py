"""The structure the engine's design rests on, held on the compiled code of csrc/sgo_engine.hip (no GPU needed).

k_search runs ONE wavefront per game with the whole GameState in registers and no calls.  Nothing in the language states that:
it holds because every device function k_search and k_debug_top_one reach is `__forceinline__` (the rule and the measurements
behind it are at the top of csrc/sgo_search.hpp).  One stage left out of line puts GameState in scratch memory -- 768 B per
lane, measured -- and the golden games still pass, only slower.  So this test compiles the device listing with build.py's flags
and checks what the source cannot promise: no call instruction, no function emitted besides the kernels, no scratch in any
kernel, and in every k_search<S> no dynamic stack and no static LDS (its LDS is the dynamic block sized by search_lds).
Register counts are NOT pinned: they move with the compiler."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (5, 7, 9, 13, 19)


def _tool():
    spec = importlib.util.spec_from_file_location("vmcnt_isa_check", os.path.join(ROOT, "tools", "vmcnt_isa_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernel_descriptors(asm):
    """{kernel symbol: {directive: value}} from the .amdhsa_kernel blocks of a device listing."""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
        out[m.group(1)] = dict(re.findall(r"^\s*(\.amdhsa_\w+)\s+(\S+)", m.group(2), re.M))
    return out


def structure_problems(asm):
    """Everything in a device listing that breaks the engine's structure, as a list of sentences (empty = sound)."""
    bad = []
    kern = kernel_descriptors(asm)
    calls = re.findall(r"^\s*(s_swappc_b64|s_call_b64)\b", asm, re.M)
    if calls:
        bad.append("%d call instruction(s) (%s): a device function was not inlined" % (len(calls), calls[0]))
    for sym in re.findall(r"^\s*\.type\s+(\S+?),@function", asm, re.M):
        if sym not in kern:
            bad.append("function %s is emitted out of line" % sym)
    for sym, d in sorted(kern.items()):
        if d.get(".amdhsa_private_segment_fixed_size") != "0":
            bad.append("%s: %s B of scratch per lane" % (sym, d.get(".amdhsa_private_segment_fixed_size")))
        if "k_search" in sym:
            if d.get(".amdhsa_uses_dynamic_stack") != "0":
                bad.append("%s: uses a dynamic stack" % sym)
            if d.get(".amdhsa_group_segment_fixed_size") != "0":
                bad.append("%s: %s B of static LDS (its LDS is dynamic only)" % (sym, d.get(".amdhsa_group_segment_fixed_size")))
    return bad


def missing_kernels(asm):
    """Kernels the engine must ship that the listing lacks: all five sizes of k_search / k_start / k_debug_top_one, and k_compact."""
    kern = kernel_descriptors(asm)
    want = ["_ZN3sgo9k_compactE"]
    for s in SIZES:
        want += ["_ZN3sgo8k_searchILi%dEE" % s, "_ZN3sgo7k_startILi%dEE" % s, "_ZN3sgo15k_debug_top_oneILi%dEE" % s]
    return [w for w in want if sum(k.startswith(w) for k in kern) != 1]


_KERNEL = """\t.type\t%(sym)s,@function
%(sym)s:
%(body)s\ts_endpgm
\t.amdhsa_kernel %(sym)s
\t\t.amdhsa_group_segment_fixed_size %(lds)d
\t\t.amdhsa_private_segment_fixed_size %(scratch)d
\t\t.amdhsa_uses_dynamic_stack %(dyn)d
\t\t.amdhsa_next_free_vgpr 32
\t.end_amdhsa_kernel
"""
_SEARCH5 = "_ZN3sgo8k_searchILi5EEEvNS_3CtxEPKfS3_iPKi"


def _listing(body="\tv_mov_b32_e32 v0, 0\n", lds=0, scratch=0, dyn=0, extra=""):
    return extra + _KERNEL % dict(sym=_SEARCH5, body=body, lds=lds, scratch=scratch, dyn=dyn)


def test_the_checker_can_fail():
    """Two small synthetic listings, one with a call and one with scratch, must both be flagged (and a sound one must not):
    otherwise a green run of the real check below would mean nothing."""
    assert structure_problems(_listing()) == []
    # the shape the move step took as a plain lambda: an out-of-line callee reached through s_swappc_b64
    callee = "_ZZN3sgo8k_searchILi5EEEvNS_3CtxEPKfS3_iPKiENKUliE_clEi"
    with_call = _listing(body="\ts_getpc_b64 s[4:5]\n\ts_swappc_b64 s[30:31], s[4:5]\n", dyn=0,
                         extra="\t.type\t%s,@function\n%s:\n\ts_setpc_b64 s[30:31]\n" % (callee, callee))
    found = structure_problems(with_call)
    assert any("call instruction" in p for p in found) and any("out of line" in p and callee in p for p in found), found
    found = structure_problems(_listing(scratch=768))
    assert found == ["%s: 768 B of scratch per lane" % _SEARCH5], found
    # and the k_search-only terms
    assert any("dynamic stack" in p for p in structure_problems(_listing(dyn=1)))
    assert any("static LDS" in p for p in structure_problems(_listing(lds=408)))
    assert len(missing_kernels(_listing())) == 1 + 3 * len(SIZES) - 1


def test_engine_kernels_are_call_free_and_scratch_free():
    asm = _tool().device_asm(source="sgo_engine.hip")
    if asm is None:
        pytest.skip("no hipcc")
    assert missing_kernels(asm) == []
    assert len(kernel_descriptors(asm)) == 1 + 3 * len(SIZES)
    assert structure_problems(asm) == []
