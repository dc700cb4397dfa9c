"""CPU-only: the ABI of the heads kernel and of the library's net object (include/sgo.h, ABI version 4) as the bindings see it.
No compute calls: there is no GPU in the CPU test tier."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sgo_heads_packed_bytes", "sgo_heads_prepack_dev", "sgo_heads_dev", "sgo_net_create", "sgo_net_set_weights",
               "sgo_net_packed_tower", "sgo_net_predict_packed_dev", "sgo_net_destroy")


def _lib():
    from sejonggo_amd.build import build_lib
    from sejonggo_amd import _lib as L
    build_lib()
    return L


def _header():
    return open(os.path.join(ROOT, "include", "sgo.h")).read()


def test_new_symbols_are_declared_listed_and_exported():
    L = _lib()
    lib = L.load()
    declared = set(re.findall(r"\b(sgo_[a-z0-9_]+)\s*\(", _header()))
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in L.SYMBOLS, s
        assert hasattr(lib, s), s
    assert "typedef struct sgo_net sgo_net;" in _header()
    assert "typedef struct sgo_net_weights {" in _header()


def test_abi_version_is_4_everywhere():
    L = _lib()
    assert L.load().sgo_version() == 4 == L.ABI_VERSION
    assert re.search(r"#define\s+SGO_ABI_VERSION\s+4\b", _header())
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "sgo_version() != 4" in integration or "sgo_version() == 4" in integration


def test_net_weights_layout_matches_header(tmp_path):
    """ctypes NetWeights against the C compiler's sizeof / offsetof of sgo_net_weights."""
    L = _lib()
    cls, cname = L.NetWeights, "sgo_net_weights"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sgo.h"', 'int main(void) {',
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for fname, _ in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls) == 15 * ctypes.sizeof(ctypes.c_void_p)
    for fname, _ in cls._fields_:
        assert int(got["%s.%s" % (cname, fname)]) == getattr(cls, fname).offset, fname
    # every field of the C struct is mirrored, in order
    body = re.search(r"typedef struct sgo_net_weights \{(.*?)\} sgo_net_weights;", _header(), re.S).group(1)
    c_fields = re.findall(r"\*\s*(?:const\s*\*\s*)?([a-z0-9_]+)\s*[,;]", body)
    assert c_fields == [f for f, _ in cls._fields_], c_fields


def test_header_still_compiles_as_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "sgo.h"\n'
                   'int main(void) { sgo_net_weights w; sgo_net *n = 0; (void)n; w.stem_w10 = 0; (void)w; return 0; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)])


def test_heads_geometry_is_host_arithmetic():
    """sgo_heads_packed_bytes needs no device: (A padded to 16, plus 256) x (2 t^2 padded to 32) fp16."""
    L = _lib()
    lib = L.load()
    for S in L.SUPPORTED_SIZES:
        t2, A = (S - 2) ** 2, S * S + 1
        kp, npad = -(-2 * t2 // 32) * 32, -(-A // 16) * 16
        assert lib.sgo_heads_packed_bytes(S) == (npad + 256) * kp * 2, S
    assert lib.sgo_heads_packed_bytes(19) == 758784
    assert lib.sgo_heads_packed_bytes(8) < 0


def test_no_cpu_fallback_without_gpu():
    """Without a HIP device NativeNet and use_fused_heads raise the library's error; nothing is computed on the CPU."""
    L = _lib()
    if L.load().sgo_device_count() > 0:
        return
    from sejonggo_amd.net import FusedInferenceNet, NativeNet, PolicyValueNet
    net = PolicyValueNet(5, 1, 256)
    net.eval()
    with pytest.raises(L.SgoError, match="no HIP device"):
        NativeNet(net, device="cpu")
    bare = object.__new__(FusedInferenceNet)          # the constructor itself refuses without a device
    with pytest.raises(L.SgoError, match="no HIP device"):
        bare.use_fused_heads(True)
    assert not L.load().sgo_net_create(9, 4, 64, 0)   # NULL + message, not a host-side net
    assert L.load().sgo_last_error()
