"""ChordPixelRaysDesc and chordvis_pixel_rays across the three places that state them: include/chordvis.h (a small C program prints
sizeof, every offsetof and the mode and flag macros), chord_amd/lib.py (the ctypes structure, the constants and the prototype) and the
specification tests/spec_pixel_rays_np.py.  No device calls (runs without a GPU)."""
import ctypes as C
import os
import subprocess

import spec_pixel_rays_np as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MACROS = ("HEMISPHERE", "DIRECTION", "ANY_HIT", "FRONT_ONLY", "START_FROM_DEPTH")
FIELDS = ("width", "height", "mode", "flags", "tableW", "tableH", "deviceZStride", "pad", "direction", "rayLength", "tMin", "zNear", "pad2")


def test_desc_layout_and_macros_match_the_header(tmp_path):
    from chord_amd import lib as L
    lines = ['printf("sizeof %zu\\n", sizeof(ChordPixelRaysDesc));']
    lines += ['printf("%s %%zu\\n", offsetof(ChordPixelRaysDesc, %s));' % (f, f) for f in FIELDS]
    lines += ['printf("%s %%u\\n", (unsigned)CHORD_PIXEL_RAYS_%s);' % (f, f) for f in MACROS]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "chordvis.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(lines)
    cpath, exe = str(tmp_path / "l.c"), str(tmp_path / "l")
    open(cpath, "w").write(src)
    cc = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-1500:]
    out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(out["sizeof"]) == 64 == C.sizeof(L.PixelRaysDesc)
    assert tuple(n for n, _ in L.PixelRaysDesc._fields_) == FIELDS
    for f in FIELDS:
        assert int(out[f]) == getattr(L.PixelRaysDesc, f).offset, f
    assert [int(out[f]) for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 44, 48, 52, 56]
    assert L.PixelRaysDesc.direction.size == 12 and L.PixelRaysDesc.pad2.size == 8
    for f in MACROS:
        assert int(out[f]) == getattr(L, "PIXEL_RAYS_" + f) == getattr(PR, f), f
    assert [int(out[f]) for f in MACROS] == [0, 1, 1, 2, 4]


def test_ctypes_prototype_is_the_headers():
    """int chordvis_pixel_rays(ChordCtx*, const ChordPixelRaysDesc*, const float*, const float*, const float*, const float*, float*,
    ChordRayHit*): eight arguments, the desc as a pointer to the structure, every other pointer a void pointer, an int back."""
    from chord_amd import lib as L
    assert "chordvis_pixel_rays" in L.EXPORTED
    fn = L.lib.chordvis_pixel_rays
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.POINTER(L.PixelRaysDesc)] + [C.c_void_p] * 6
    hdr = open(os.path.join(ROOT, "include", "chordvis.h")).read()
    decl = hdr[hdr.index("int chordvis_pixel_rays("):]
    decl = " ".join(decl[:decl.index(";")].split())
    assert decl == ("int chordvis_pixel_rays(ChordCtx* ctx, const ChordPixelRaysDesc* desc, const float* devicePosition /* float4 */, "
                    "const float* deviceNormal /* float4 */, const float* deviceZ /* or NULL */, "
                    "const float* deviceTable /* float4, HEMISPHERE only */, float* deviceOut /* float */, "
                    "ChordRayHit* deviceHits /* or NULL */)"), decl
    # a null context is refused before anything is looked at
    assert fn(None, None, None, None, None, None, None, None) == L.E_INVALID
