"""Regenerates gltf_library_mesh.npz and gltf_library_check.json: files the LIBRARY writes (chordvis_save_gltf_binary, uncompressed
and LZ4) from a fixed mesh, read back by loadAsset's sequence built from the reference's vendored cereal + LZ4
(make_gltf_binary_fixture.cpp --check).  The JSON keeps each file's size and SHA-1 beside what the reference's reader reported, so
tests/test_nanite_builder.py holds the library to it without the reference's sources.

    python tests/golden/make_gltf_library_fixture.py REFERENCE_EXTERNAL_DIR

REFERENCE_EXTERNAL_DIR: the reference's `external` directory (include/cereal, lz4/lib); its sources are compiled where they lie,
nothing of them is copied."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

from chord_amd import lib as L, scenes  # noqa: E402

MESH = os.path.join(HERE, "gltf_library_mesh.npz")
OUT = os.path.join(HERE, "gltf_library_check.json")


def main(ref):
    pos, idx, uv = scenes.bumpy_sphere_mesh(48, 3)
    np.savez_compressed(MESH, positions=pos, indices=idx, texcoords0=uv)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "check")
        subprocess.run(["g++", "-O1", "-std=c++17", "-I", ref + "/include", "-I", ref + "/lz4/lib", os.path.join(HERE, "make_gltf_binary_fixture.cpp"),
                        ref + "/lz4/lib/lz4.c", "-o", exe], check=True)
        h = L.nanite_build(pos, idx, uv, keep_handle=True)
        files = []
        for lz4 in (0, 1):
            path = os.path.join(tmp, "w%d.bin" % lz4)
            assert L.lib.chordvis_save_gltf_binary(h, path.encode(), lz4) == L.OK
            data = open(path, "rb").read()
            out = subprocess.run([exe, "--check", path], capture_output=True, text=True, check=True).stdout.strip()
            files.append({"lz4": lz4, "bytes": len(data), "sha1": hashlib.sha1(data).hexdigest(), "reference_check": out})
        L.lib.chordvis_free_built_asset(h)
    with open(OUT, "w") as fh:
        json.dump({"mesh": os.path.basename(MESH), "files": files}, fh, indent=1)
        fh.write("\n")
    print(json.dumps(files, indent=1))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
