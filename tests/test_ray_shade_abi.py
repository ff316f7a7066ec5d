"""ChordRayHitSurface and chordvis_shade_ray_hits across the three places that state them: include/chordvis.h (a small C program
prints sizeof, every offsetof and the flag macros), chord_amd/records.py + chord_amd/lib.py (the numpy record, the constants and the
ctypes prototype) and the specification tests/spec_ray_shade_np.py.  No device calls (runs without a GPU)."""
import ctypes as C
import os
import subprocess

from chord_amd import records as R

import spec_ray_shade_np as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("VALID", "BACK_FACE", "TWO_SIDED", "PBR")


def test_record_layout_and_flags_match_the_header(tmp_path):
    dt = R.RAY_HIT_SURFACE
    lines = ['printf("sizeof %zu\\n", sizeof(ChordRayHitSurface));', 'printf("hit %zu\\n", sizeof(ChordRayHit));']
    lines += ['printf("%s %%zu\\n", offsetof(ChordRayHitSurface, %s));' % (f, f) for f in dt.names]
    lines += ['printf("%s %%u\\n", (unsigned)CHORD_RAYSURF_%s);' % (f, f) for f in FLAGS]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "chordvis.h"\nint main(void){\n%s\nreturn 0;}\n' % "\n".join(lines)
    cpath, exe = str(tmp_path / "l.c"), str(tmp_path / "l")
    open(cpath, "w").write(src)
    cc = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), cpath, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-1500:]
    out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(out["sizeof"]) == 64 == dt.itemsize == RS.RAY_HIT_SURFACE.itemsize and int(out["hit"]) == R.RAY_HIT.itemsize
    assert dt == RS.RAY_HIT_SURFACE and dt.names == RS.RAY_HIT_SURFACE.names
    assert dt.names == ("baseColor", "emissive", "roughness", "normal", "metallic", "uv", "material", "flags")
    for f in dt.names:
        assert int(out[f]) == dt.fields[f][1] == RS.RAY_HIT_SURFACE.fields[f][1], f
        assert dt.fields[f][0] == RS.RAY_HIT_SURFACE.fields[f][0], f
    from chord_amd import lib as L
    for f in FLAGS:
        assert int(out[f]) == getattr(L, "RAYSURF_" + f) == getattr(RS, "RAYSURF_" + f), f
    assert [int(out[f]) for f in FLAGS] == [1, 2, 4, 8]


def test_ctypes_prototype_is_the_headers():
    """int chordvis_shade_ray_hits(ChordCtx*, const ChordRayHit*, uint32_t, float, const float*, ChordRayHitSurface*): six arguments,
    the float as a float in fourth place, every pointer a void pointer, an int back."""
    from chord_amd import lib as L
    assert "chordvis_shade_ray_hits" in L.EXPORTED
    fn = L.lib.chordvis_shade_ray_hits
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    hdr = open(os.path.join(ROOT, "include", "chordvis.h")).read()
    decl = hdr[hdr.index("int chordvis_shade_ray_hits("):]
    decl = " ".join(decl[:decl.index(";")].split())
    assert decl == ("int chordvis_shade_ray_hits(ChordCtx* ctx, const ChordRayHit* deviceHits, uint32_t count, float lod, const float* deviceLods, "
                    "ChordRayHitSurface* deviceSurfaces)"), decl
    # a null context is refused before anything is looked at
    assert fn(None, None, 0, 0.0, None, None) == L.E_INVALID
