"""chordvis_material_feedback (include/chordvis.h ChordFeedbackDesc) restated in numpy: per texture and level, how many lattice pixels'
finest tap landed there.  Nothing is computed here that spec_material_np / spec_material_aniso_np do not already report: the counts
are a histogram of their `stats` (slots[slot][i]["pix"], ["l0"]) over the pixels of the lattice.  Also the helper that presents a
scene with textures trimmed as chordvis_set_texture_first_level stores them.  TEST INFRASTRUCTURE: never imported by chord_amd/."""
import numpy as np

import spec_material_aniso_np as SA
import spec_material_np as SM

LEVELS = 16                                      # CHORD_FEEDBACK_LEVELS
SLOT_BITS = {"baseColor": 1, "emissive": 2, "normal": 4, "metallicRoughness": 8}     # CHORD_FEEDBACK_*, in SM.SLOTS' order


def resolve_stats(scene, vis, cmds, view, iv, w, h, max_aniso=1):
    """the sampler statistics of one frame under one anisotropy: computed once, shared by every feedback() of that frame"""
    stats = {}
    if max_aniso == 1:
        SM.resolve(scene, vis, cmds, view, iv, w, h, stats=stats)
    else:
        SA.resolve(scene, vis, cmds, view, iv, w, h, stats=stats, max_aniso=max_aniso)
    return stats


def on_lattice(pix, w, stride, offset):
    pix = np.asarray(pix, dtype=np.int64)
    return ((pix % w) % stride == offset[0]) & ((pix // w) % stride == offset[1])


def feedback_of(stats, scene, w, slot_mask=15, stride=1, offset=(0, 0)):
    """(textureCount, 16) uint32 from resolve_stats' result"""
    taps = np.zeros((len(scene.texture_images), LEVELS), dtype=np.int64)
    for slot in SM.SLOTS:
        if not slot_mask & SLOT_BITS[slot]:
            continue
        for st in stats["slots"][slot]:
            tid = int(scene.materials[st["material"]][SM._TEX_FIELD[slot][0]])
            keep = on_lattice(st["pix"], w, stride, offset)
            taps[tid] += np.bincount(np.asarray(st["l0"], dtype=np.int64)[keep], minlength=LEVELS)
    return (taps & 0xFFFFFFFF).astype(np.uint32)


def feedback(scene, vis, cmds, view, iv, w, h, slot_mask, stride, offset, max_aniso=1):
    return feedback_of(resolve_stats(scene, vis, cmds, view, iv, w, h, max_aniso), scene, w, slot_mask, stride, offset)


def pairs_on_lattice(stats, w, slot_mask=15, stride=1, offset=(0, 0)):
    """how many (PBR hit pixel on the lattice, slot of the mask with a texture) pairs the frame has"""
    return sum(int(on_lattice(st["pix"], w, stride, offset).sum())
               for slot in SM.SLOTS if slot_mask & SLOT_BITS[slot] for st in stats["slots"][slot])


def finished_levels(scene, tid):
    """the (h, w, 4) uint8 levels of an RGBA8 texture of `scene` as supplied"""
    chain, mips = scene._tex_chains[tid]
    img = scene.texture_images[tid]
    assert getattr(img, "format", 0) == 0, "trimmed(): RGBA8 textures only (decode block chains first)"
    out, off = [], 0
    for l in range(mips):
        lw, lh = max(1, img.shape[1] >> l), max(1, img.shape[0] >> l)
        out.append(np.asarray(chain[off:off + lw * lh * 4], dtype=np.uint8).reshape(lh, lw, 4))
        off += lw * lh * 4
    return out


def trimmed(scene, first, levels_of=None):
    """`scene` as chordvis_set_texture_first_level(first) leaves its material textures: texture i is the RGBA8 chain of levels
    min(first[i], L - 1) .. L - 1 of its finished chain (levels_of[i]: that chain when the library makes or decodes levels; default:
    the supplied one)."""
    from chord_amd import records as R, scenes
    out = []
    for i in range(len(scene.texture_images)):
        lv = levels_of[i] if levels_of is not None and levels_of.get(i) is not None else finished_levels(scene, i)
        f = min(int(first[i]) if i < len(first) else 0, len(lv) - 1)
        kept = lv[f:]
        out.append(R.TextureChain(np.concatenate([np.ascontiguousarray(l).reshape(-1) for l in kept]), kept[0].shape[1], kept[0].shape[0], len(kept), 0))
    return scenes.with_textures(scene, out)
