"""The TLAS rebuild's part of the C ABI: the two entry points are declared, exported and prototyped alike; CHORD_RAY_TLAS_GROUP_MAX
and the child-word tags of chord_amd/lib.py are the header's; records.RAY_NODE is ChordRayNode field for field.  No device calls."""
import ctypes as C
import os
import re
import subprocess

from chord_amd import lib as L, records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_entry_points_are_declared_exported_and_prototyped():
    hdr = _header("chordvis.h")
    assert re.search(r"\bint\s+chordvis_rebuild_ray_tlas\s*\(\s*ChordCtx\s*\*\s*ctx\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+chordvis_readback_ray_tlas\s*\(\s*ChordCtx\s*\*\s*ctx\s*,\s*ChordRayNode\s*\*\s*hostNodes\s*,\s*uint32_t\s+nodeCapacity\s*,"
                     r"\s*uint32_t\s*\*\s*hostLeafRef\s*,\s*uint32_t\s+objectCapacity\s*\)\s*;", hdr)
    for name, args in (("chordvis_rebuild_ray_tlas", [C.c_void_p]),
                       ("chordvis_readback_ray_tlas", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32])):
        assert name in L.EXPORTED
        fn = getattr(L.lib, name)
        assert fn.restype is C.c_int32 or fn.restype is C.c_int
        assert list(fn.argtypes) == args, name
    # a NULL context is refused without touching a device
    assert L.lib.chordvis_rebuild_ray_tlas(None) == L.E_INVALID
    assert L.lib.chordvis_readback_ray_tlas(None, None, 0, None, 0) == L.E_INVALID


def test_macros_and_node_layout_match_the_header(tmp_path):
    types = _header("chordvis_types.h")
    value = lambda name: int(re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, types).group(1), 0)
    assert value("CHORD_RAY_TLAS_GROUP_MAX") == L.RAY_TLAS_GROUP_MAX
    assert (value("CHORD_RAY_TLAS_NODE"), value("CHORD_RAY_TLAS_LEAF"), value("CHORD_RAY_NO_CHILD")) == (L.RAY_TLAS_NODE, L.RAY_TLAS_LEAF, L.RAY_NO_CHILD)
    g = L.RAY_TLAS_GROUP_MAX            # 0: one path for every count; otherwise what the one-workgroup kernel is built for
    assert g == 0 or (g % 1024 == 0 and g & (g - 1) == 0 and g * 8 + 64 <= 65536)
    lines = ['printf("size %zu\\n", sizeof(ChordRayNode));'] + \
            ['printf("%s %%zu\\n", offsetof(ChordRayNode, %s));' % (f, f) for f in R.RAY_NODE.names]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "chordvis.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(lines)
    cpath, exe = str(tmp_path / "n.c"), str(tmp_path / "n")
    open(cpath, "w").write(src)
    cc = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-1500:]
    out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(out["size"]) == R.RAY_NODE.itemsize == 128
    for f in R.RAY_NODE.names:
        assert int(out[f]) == R.RAY_NODE.fields[f][1], f
    assert R.RAY_NODE["lo"].shape == (3, 4) and R.RAY_NODE["child"].shape == (4,)
