"""What the tests of ptamd_scene_update_materials share (tests/test_materials_{cpu,gpu}.py): the scene of tests/replace_cases.py taken
through a list of changes of its material table, texture descriptors, texel blob and material ids.  A step names only what it
changes; `changed` forms the descriptor the call's contract names (the old one with those substituted)."""
import numpy as np

from replace_cases import material_scene, mixed_ids

# The scene of replace_cases: textures 0 and 1 are 1x1 RGBA (floats 0..3, 4..7), 2 a 4x4 RGBA map (8..71), 3 a 4x4 RGB normal map
# (72..119); materials m0 = (0, -1, 1.0) flat, m1 = (1, -1, 1.5), m2 = (2, 3, 1.0)
BLOB = 120
COUNTS = (1, 255, 256, 257, 300, 500)   # one group, its boundary, a one-thread last group; compact; beyond the compact layout
FIFTH = np.array([0.15, 0.85, 0.35, 0.6], np.float32)


def changed(P, hs, materials=None, textures=None, texels=None, ids=None):
    """`hs` with the given tables (whole) substituted; ids: per face"""
    f = hs.faces.copy()
    if ids is not None:
        f["material_id"] = np.asarray(ids, np.uint32)
    return P.HostScene(f, hs.mesh_sizes, hs.materials if materials is None else materials, hs.lights,
                       hs.textures if textures is None else textures, hs.texels if texels is None else texels, hs.camera, hs.cubemap)


def with_material(P, hs, index, **fields):
    m = hs.materials.copy()
    for k, v in fields.items():
        m[k][index] = v
    return m


def transitions(P, n):
    """[(what, {materials, textures, texels (the whole new blob), ids} as the step changes them)] in the order they are applied, from
    material_scene(P, n) with every face on m0.  Every step is seen in the records of some face for n > 1."""
    base = material_scene(P, n)
    tex28 = base.textures.copy()
    tex28["w"][2], tex28["h"][2] = 2, 8
    tex5 = np.concatenate([tex28, np.array([(1, 1, 4, 0, BLOB)], dtype=P.TEXTURE_DTYPE)])
    blob5 = np.concatenate([base.texels, FIFTH])
    one = lambda **f: with_material(P, base, 0, **f)
    return [
        ("all m0 to mixed ids", dict(ids=mixed_ids(n))),
        ("mixed ids to all m0", dict(ids=np.zeros(n, np.uint32))),
        ("m0's map 0 to 1", dict(materials=one(diffuse_spec_map=1))),
        ("m0's ior 1.0 to 1.5", dict(materials=one(diffuse_spec_map=1, ior=1.5))),
        ("m0's ior to NaN", dict(materials=one(diffuse_spec_map=1, ior=np.nan))),
        ("mixed ids again", dict(ids=mixed_ids(n))),
        ("the 4x4 map re-described as 2x8", dict(textures=tex28)),
        ("a fifth texture behind a longer blob, named by m0", dict(materials=one(diffuse_spec_map=4), textures=tex5, texels=blob5)),
        ("one material, every id 0", dict(materials=one(diffuse_spec_map=4)[:1], ids=np.zeros(n, np.uint32))),
    ]


def states(P, n):
    """[(what, step, the scene before, the scene after)] along transitions(P, n)"""
    hs, out = material_scene(P, n), []
    for what, step in transitions(P, n):
        new = changed(P, hs, **step)
        out.append((what, step, hs, new))
        hs = new
    return out
