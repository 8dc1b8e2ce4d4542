"""One scene id taken through long, mixed sequences of the calls that change an uploaded scene (DESIGN.md §13 "Sequences"):
the host's statement of what the id holds after each call (Model), the sequences, the rays, and the comparisons.  No GPU here.
tests/test_sequence_cpu.py checks what the GPU test rests on, tests/test_sequence_gpu.py runs the sequences on the device.

The invariant: whatever the history of a scene id, every reader answers as the CPU oracle, or the reader's host mirror, answers for
the descriptor the scene holds NOW.  So the model keeps that descriptor and little else; every op kind is one method that advances it
with the host functions the per-call suites already pin (P.deform, host_pose_faces, host_skin_faces, host_morph_faces,
materials_cases.changed / with_material, replace_cases.replaced) and returns the arguments of the device call.

What the model carries beside the descriptor, and why (test_sequence_cpu.py checks that nothing more is needed):
  built_from   the faces the scene's tree was built from and by which path: the link table after a relink is
               host_relink_words(built_from, refit_to=now), and the layout (compact or not, a link table or none) is the tree's
  culled       whose faces the link table's culled links stand for: the tree's own ("built"), the host update's ("host"), a relink's
               ("relink") or nobody's ("none": every update from device faces puts the plain table back)
  rig          the rest faces of the open rig, or the fact that it is of an older count and must be refused and reopened
A refit is memoryless (host_scene_tables(s, a, b) == host_scene_tables(s, b)) and tables 3 and 4 are in storage order, so no other
history is kept.

Geometry ops move the faces by a fifth of an edge or less: every comparison is exact, so the smallest motion shows a stale reader, and the
rays (aimed at the faces of the start scene) keep hitting what they were aimed at.

The pairs of op kinds the contract forbids (FORBIDDEN) still occur in the sequences: the model exercises each as a refusal that
changes nothing, then reopens the rig and goes on."""
import numpy as np

import materials_cases as MC
import query_cases as QC
import rig_cases as RC
from helpers import random_rays
from replace_cases import material_scene, mixed_ids, replaced

KINDS = ("update_host", "update_device", "rebuild", "rebuild_finish", "replace", "replace_finish", "materials", "texels", "pose", "skin",
         "morph", "lights", "relink")
RIG = ("pose", "skin", "morph")
GEOMETRY = ("update_host", "update_device", "rebuild", "rebuild_finish", "replace", "replace_finish") + RIG
DEVICE_SIDE = ("update_device", "rebuild", "rebuild_finish", "replace", "replace_finish", "relink") + RIG   # the host never sees the faces
STARTS = ("grid300", "indoor", "grid37", "grid500", "gridT200")

# include/ptamd.h, "Another number of faces", "What follows for the other calls":
RIG_OF_ANOTHER_COUNT = ("A rig made for another count is refused at its next pose, skin or morph with PTAMD_ERR_ARG (it can still be "
                        "destroyed)")
FORBIDDEN = {(a, b): RIG_OF_ANOTHER_COUNT for a in ("replace", "replace_finish") for b in RIG}

SIZE, SPP, BOUNCES = (48, 48), 2, 3
N_RANDOM, N_LIGHTS, N_FAR, N_HOSTILE = 1024, 64, 128, 64        # 1 280 rays: at least kQueryResidentMinRays
N_RAYS = N_RANDOM + N_LIGHTS + N_FAR + N_HOSTILE
N_BONES, SEQUENCE_OPS = 5, 14                                   # (ops cut from the circuit; two more where the far light is brought back)
FAR_LIGHT = 3.0e4                                               # beyond the margins' reach: launches test every face
# query_cases.check_not_vacuous asks of 4 736 rays: 5 light hits with and without ranges, 200 of 512 far-origin rays on a face, a
# mixed ANY mask.  Here, of 1 280: 2 light hits without ranges (5 * 1 280 / 4 736 = 1.35, rounded up; the sphere test takes a
# direction for a unit vector, so of the aimed rays only those about one unit long hit), 1 with ranges (the rays aimed again after a
# lights op keep the ranges of the start, which were not derived for them), 50 of 128 far-origin rays (the same share), a mixed mask
MIN_LIGHT_HITS, MIN_LIGHT_HITS_IN_RANGE, MIN_FAR_HITS = 2, 1, 50
# ... and what makes a step seen: the frame in 1 % of its pixels, the query records of a geometry step on 5 % of the rays, those of
# a lights step on 16 rays by kind or index (a light hit that moves by a bit of t does not count)
MIN_PIXEL_SHARE, MIN_RAY_SHARE, MIN_LIGHT_RAYS = 0.01, 0.05, 16
PITCH = 3.0 / 64                                                # rebuild_cases.grid_tris
MOTION = 0.2                                                    # of an edge: how far a geometry op moves a vertex, about


def group_prims(P):
    return int(P.native.load().ptamd_build_group_prims())


def start_scene(P, name):
    """replace_cases.material_scene at the smallest counts where the code changes path (37: tiny and compact; 300: compact,
    LDS-resident, flat and skip forms; 500: beyond the compact layout, the four-wide walk; kBuildGroupPrims + 200: the device
    builder), and indoor: resident, its upload builds a skip set and culls."""
    if name == "indoor":
        import os
        from conftest import ASSETS
        return P.HostScene.load(os.path.join(ASSETS, "indoor.scene"))
    n = {"grid37": 37, "grid300": 300, "grid500": 500, "gridT200": group_prims(P) + 200}[name]
    return material_scene(P, n)


def replace_target(P, name, j):
    """The faces the j-th replace of a sequence goes to.  A replace always changes the count, a sequence crosses the compact layout's
    boundary in both directions, and no count comes twice in a sequence (j more faces each time, or j fewer), so a rig opened before
    a replace is always of another count after it.  Every grid has the layout and the seed of the start's, so the rays aimed at the
    start's faces go on hitting; 37 faces are a start only (too few of a larger start's rays are aimed at them).  indoor goes to
    its faces split in four (the device builder), back, and to every other face, each deformed a little."""
    if name == "indoor":
        from cuda_pathtracer_amd.synthetic import tessellate
        hs = start_scene(P, name)
        # (split faces alone would look as before: each target is moved and shaded a little differently too)
        f = (tessellate(hs, 2), hs, replaced(P, hs, hs.faces[::2]))[j % 3]
        return P.deform(f, 1.1 + j, 0.05, shading=True).faces[: len(f.faces) - 1 - j].copy()
    return material_scene(P, (500, 300, group_prims(P) + 200)[j % 3] + 1 + j).faces


def layout_of(P, hs, how):
    """What the tree over `hs` is, by the path that built it ("upload", or a rebuild / replace): dict(resident, links, culled, how).
    A rebuilt tree is the binned one unless that takes the compact layout, which the upload's builder then builds (include/ptamd.h)."""
    n = len(hs.faces)

    def fits(t):
        nodes, tris = t["nodes"].size // 64, t["tris_bvh"].size // 48
        return nodes * 64 + tris * 48 <= 64 * 1024 and nodes <= 896 and n <= 2047

    if how != "upload":
        if not fits(P.host_rebuild_tables(hs, hs.faces)):
            return dict(resident=False, links=False, culled=0, how="device" + ("_finish" if how.endswith("finish") else ""))
        how = "host"
    if not fits(P.host_scene_tables(hs)):
        return dict(resident=False, links=False, culled=0, how=how)
    skipped = int(P.host_skip_trace(hs, np.zeros((0, 6), np.float32), mode="default", cull=True)["skip"].sum())
    culled = P.host_relink_words(hs)[1]
    return dict(resident=True, links=skipped + culled > 0, culled=culled, how=how)


def small_transforms(n, seed, centre, reach, edge):
    """n rigid transforms float32[n, 3, 4]: a rotation about a tilted axis through `centre` that moves nothing by more than about
    MOTION of `edge`, and a translation of a quarter of that"""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, np.float64)
    t = np.zeros((n, 3, 4), np.float64)
    for g in range(n):
        r = RC.rotation((0.3, 1.0, 0.2 + 0.1 * (g % 3)), rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0]) * MOTION * edge / reach)
        t[g, :, :3] = r
        t[g, :, 3] = c - r @ c + rng.uniform(-0.25, 0.25, 3) * MOTION * edge
    return t.astype(np.float32)


class Model:
    """What one scene id holds (see the module's text).  Every op kind is a method that advances the model and returns the device
    call's arguments as a dict; scene() is the descriptor of now."""

    def __init__(self, P, start, mixed=False):
        """mixed: a grid starts under replace_cases.mixed_ids (not flat) instead of all m0"""
        self.P, self.start, self.grid = P, start, start != "indoor"
        hs = start_scene(P, start)
        self.materials, self.textures, self.texels, self.lights = hs.materials.copy(), hs.textures.copy(), hs.texels.copy(), hs.lights.copy()
        self.materials0, self.lights0, self.camera0, self.cubemap = hs.materials.copy(), hs.lights.copy(), hs.camera.copy(), hs.cubemap
        self.alt_ids, self.alt_table, self.far = bool(mixed) and self.grid, False, False
        self.replaces = 0
        self._set_base(hs.faces, hs.mesh_sizes)
        self.built_from, self.built_how, self.culled = self.scene(), "upload", "built"
        self.rig = self._open_rig()           # opened behind the upload
        self.steps, self.count = 0, {k: 0 for k in KINDS}
        self._layouts = {}

    # ---- the descriptor
    def _set_base(self, faces, mesh_sizes):
        self.base = np.ascontiguousarray(faces, dtype=self.P.FACE_DTYPE).copy()
        self.faces, self.own_ids, self.mesh_sizes = self.base.copy(), self.base["material_id"].copy(), np.asarray(mesh_sizes, np.uint32).copy()
        v = self.base["vertices"].astype(np.float64)
        self.edge = float(np.median(np.linalg.norm(v - np.roll(v, 1, axis=1), axis=2)))
        self.centre = v.reshape(-1, 3).mean(axis=0)
        self.reach = float(np.linalg.norm(v.reshape(-1, 3) - self.centre, axis=1).max())
        n = len(self.base)
        self.sizes = np.array([n // 2, n - n // 2], np.uint32) if len(self.mesh_sizes) == 1 else self.mesh_sizes.copy()
        self.camera = self.camera0.copy()
        if self.grid:
            # the first columns of the first rows from close by: twelve by up to twelve faces of some five pixels of 48 x 48 each, of
            # fewer than four rows six columns from half as far
            rows = min((n + 63) // 64, 12)
            cols = 12 if rows >= 4 else 6
            self.camera["position"] = (-1.5 + cols * PITCH / 2, -1.2 + rows * PITCH / 2, 0.8 * cols * PITCH)
            self.camera["aperture"], self.camera["focus_dist"] = 0.002, 0.8 * cols * PITCH

    def ids(self):
        if not self.alt_ids:
            return self.own_ids
        return mixed_ids(len(self.base)) if self.grid else ((self.own_ids + 1) % len(self.materials)).astype(np.uint32)

    def scene(self, faces=None):
        f = (self.faces if faces is None else faces).copy()
        f["material_id"] = self.ids()
        return self.P.HostScene(f, self.mesh_sizes, self.materials, self.lights, self.textures, self.texels, self.camera, self.cubemap)

    def layout(self):
        key = id(self.built_from)
        if key not in self._layouts:
            self._layouts[key] = (self.built_from, layout_of(self.P, self.built_from, self.built_how))   # (the scene is kept: its id stays its own)
        return self._layouts[key][1]

    def expected_cull(self):
        """ptamd_scene_cull_count: 0 after any update from device faces; the mirror's n_culled after a relink and after a host
        update (which culls again only where the tree's builder culled something: include/ptamd.h "CULLED LEAVES")"""
        lay = self.layout()
        if not lay["links"] or self.culled == "none":
            return 0
        if self.culled == "built":
            return lay["culled"]
        if self.culled == "host" and lay["culled"] == 0:
            return 0
        return self.P.host_relink_words(self.built_from, refit_to=self.faces)[1]

    def expected_links(self):
        """the link table after a relink (None: the scene has none)"""
        return self.P.host_relink_words(self.built_from, refit_to=self.faces)[0] if self.layout()["links"] else None

    # ---- the ops
    def _step(self, kind, **call):
        self.steps += 1
        self.count[kind] += 1
        return dict(kind=kind, **call)

    def _t(self):
        return 0.4 + 0.9 * self.steps

    def _moved(self):
        return self.P.deform(self.scene(self.base), self._t(), MOTION * self.edge, shading=True).faces

    def update_host(self):
        self.faces, self.culled = self._moved(), "host"
        return self._step("update_host", scene=self.scene())

    def update_device(self):
        self.faces, self.culled = self._moved(), "none"
        return self._step("update_device", scene=self.scene())

    def _rebuild(self, kind):
        self.faces = self._moved()
        self.built_from, self.built_how, self.culled = self.scene(), kind, "built"
        return self._step(kind, scene=self.scene(), finish=kind.endswith("finish"))

    def rebuild(self):
        return self._rebuild("rebuild")

    def rebuild_finish(self):
        return self._rebuild("rebuild_finish")

    def _replace(self, kind):
        new = replace_target(self.P, self.start, self.replaces)
        self.replaces += 1
        assert len(new) != len(self.base) and len(new) != len(self.rig["rest"])
        was = self.scene()
        self._set_base(new, [len(new)])
        now = replaced(self.P, was, self.scene())        # (the descriptor the contract names: the old one, these faces as one mesh)
        self.built_from, self.built_how, self.culled = now, kind, "built"
        return self._step(kind, scene=now, finish=kind.endswith("finish"))

    def replace(self):
        return self._replace("replace")

    def replace_finish(self):
        return self._replace("replace_finish")

    def materials_(self):
        """tables and / or ids, in turn: the ids between the faces' own and a mix (a grid's: all m0 and replace_cases.mixed_ids,
        which flips flatness both ways), the table between the upload's and one with m0's map changed (indoor: its most used
        material's map, and an ior that ends flatness)"""
        turn = self.count["materials"] % 3
        was = self.scene()
        call = {}
        if turn in (0, 2):
            self.alt_ids = not self.alt_ids
            call["ids"] = self.ids().copy()
        if turn in (1, 2):
            self.alt_table = not self.alt_table
            if not self.alt_table:
                self.materials = self.materials0.copy()
            elif self.grid:
                self.materials = MC.with_material(self.P, was, 0, diffuse_spec_map=1)
            else:
                self.materials = MC.with_material(self.P, was, 5, diffuse_spec_map=4, ior=1.5)
            call["materials"] = self.materials.copy()
        now = MC.changed(self.P, was, materials=call.get("materials"), ids=call.get("ids"))
        assert now.faces.tobytes() == self.scene().faces.tobytes() and now.materials.tobytes() == self.materials.tobytes()
        return self._step("materials", **call)

    def texels_(self):
        """the asynchronous range path: the first 24 floats of the blob (every 1x1 map of either scene), from the host and from the
        device in turn"""
        values = np.random.default_rng(500 + self.steps).uniform(0.05, 0.95, 24).astype(np.float32)
        blob = self.texels.copy()
        blob[:24] = values
        self.texels = MC.changed(self.P, self.scene(), texels=blob).texels
        return self._step("texels", values=values, first=0, device=bool(self.count["texels"] & 1))

    def _open_rig(self):
        """a rig of the faces the scene was last given (upload or replace), with a skin and morph targets (vertex deltas within a
        tenth of an edge each) attached at once"""
        n = len(self.base)
        return dict(rest=self.base.copy(), sizes=self.sizes.copy(), skin=RC.make_skin(17, n, N_BONES) + (N_BONES,),
                    targets=RC.make_targets(23, n, 2.0 * self.edge), centre=self.centre, reach=self.reach, edge=self.edge)

    def _rig(self):
        """(the rig the op uses, "refused" where the rig open until now is of another count than the scene's, i.e. was opened
        before a replace: the call is then refused and the rig reopened for the faces of now)"""
        how = None
        if len(self.rig["rest"]) != len(self.base):
            how, self.stale_groups, self.rig = "refused", len(self.rig["sizes"]), self._open_rig()
        return self.rig, how

    def _rig_call(self, kind, how, moved, **call):
        """positions come from the rig, material words from the scene"""
        r = self.rig
        self.faces, self.culled = moved.faces, "none"
        return self._step(kind, rig=how, rest=self.scene(r["rest"]), sizes=r["sizes"], skin=r["skin"], targets=r["targets"], **call)

    def pose(self):
        r, how = self._rig()
        t = small_transforms(len(r["sizes"]), 700 + self.steps, r["centre"], r["reach"], r["edge"])
        # (the call that is refused carries one transform per group of the rig it is made on, so that only the count is wrong)
        refused = {"refused_transforms": RC.identity(self.stale_groups)} if how else {}
        return self._rig_call("pose", how, self.P.host_pose_faces(self.scene(r["rest"]), t, None, r["sizes"]), transforms=t, **refused)

    def skin(self):
        r, how = self._rig()
        t = small_transforms(N_BONES, 800 + self.steps, r["centre"], r["reach"], r["edge"])
        return self._rig_call("skin", how, self.P.host_skin_faces(self.scene(r["rest"]), *r["skin"][:2], t, None), transforms=t)

    def morph(self):
        r, how = self._rig()
        w = RC.make_weights(900 + self.steps, len(r["targets"]))
        return self._rig_call("morph", how, self.P.host_morph_faces(self.scene(r["rest"]), r["targets"], w), weights=w)

    def lights_(self):
        """the first of a sequence sets light 0 beyond the margins' reach (launches then test every face), the next brings it back;
        all but the first move every light by one and a half of its radius and make it larger"""
        k = self.count["lights"]
        new = self.lights0.copy()
        self.far = k == 0
        if self.far:
            new["vec"][0], new["radius"][0] = (0.0, 0.0, FAR_LIGHT), 0.5 * FAR_LIGHT     # (of the rays aimed at it, those 0.87 units long or longer hit it)
        else:
            way = np.float32([(0.7, -0.6, 0.5), (-0.6, 0.5, -0.7), (0.5, 0.7, 0.6)][k % 3])
            new["vec"] += (np.float32(1.5) * new["radius"][:, None] * way / np.linalg.norm(way)).astype(np.float32)
            new["radius"] *= np.float32(2.0 if k & 1 else 1.5)
        self.lights = new
        return self._step("lights", lights=new.copy(), far=self.far)

    def relink(self):
        if self.layout()["links"]:
            self.culled = "relink"
        return self._step("relink")

    def apply(self, kind):
        return getattr(self, {"materials": "materials_", "texels": "texels_", "lights": "lights_"}.get(kind, kind))()


# ---------------------------------------------------------------- the sequences

def euler_circuit():
    """One closed walk over KINDS that takes every ordered pair (a, b), a == b included, exactly once (Hierholzer over the complete
    directed graph with loops, successors tried in a rotation that depends on the node): 169 pairs, 170 ops."""
    n = len(KINDS)
    left = {a: [(a + 1 + 5 * j) % n for j in range(n)] for a in range(n)}      # (5 and 13 are coprime: every successor once)
    stack, out = [0], []
    while stack:
        a = stack[-1]
        if left[a]:
            stack.append(left[a].pop(0))
        else:
            out.append(stack.pop())
    return [KINDS[k] for k in reversed(out)]


class Sequence:
    def __init__(self, index, start, kinds):
        self.index, self.start, self.kinds = index, start, tuple(kinds)
        self.mixed = start != "indoor" and bool(index & 1)      # every other grid starts not flat, so that flatness flips both ways

    def __repr__(self):
        return f"{self.index}:{self.start}{'/mixed' if self.mixed else ''}:" + ",".join(self.kinds)


def sequences():
    """The fixed list: the circuit cut into walks of SEQUENCE_OPS ops, each beginning with the op the one before ended with, so that
    no pair is lost at a cut; the starts in rotation.  A sequence's first lights op sets the far light, under which launches test
    every face and no longer show the tree: where the walk has no second lights op, "update_device, lights" is put in behind the
    first (one update meets the far light with its margins pending, the next op the walk again; no pair of the walk is parted)."""
    walk = euler_circuit()
    assert len(walk) == len(KINDS) ** 2 + 1
    step = SEQUENCE_OPS - 1
    out = []
    for i, k in enumerate(range(0, len(walk) - 1, step)):
        kinds = walk[k:k + SEQUENCE_OPS]
        if kinds.count("lights") == 1:
            at = kinds.index("lights") + 1
            kinds[at:at] = ["update_device", "lights"]
        out.append(Sequence(i, STARTS[i % len(STARTS)], kinds))
    return out


# ---------------------------------------------------------------- rays

class Rays:
    """One fixed set of 1 280 rays per start scene by query_cases' builders: 1 024 of helpers.random_rays, 64 aimed at the lights, the
    first 128 random ones from 3e4 units back, 64 hostile ones; a t_range per ray by query_cases.ranges_for from the oracle on the
    start scene.  The faces are small, so three of four random rays keep their origin and length and are turned towards a face of
    the start scene (from its front: the one from behind is taken from the other side): the first 128, the ones the far-origin rays
    repeat, towards the first 37 faces, which every grid of a sequence has."""

    def __init__(self, P, O, hs):
        rng, rest = np.random.default_rng(83), np.random.default_rng(1083)
        random = random_rays(rng, N_RANDOM, extent=3.0 if len(hs.mesh_sizes) == 1 else 3.5)
        v = hs.faces["vertices"].astype(np.float64)
        centroid, normal = v.mean(axis=1), np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        i = np.arange(N_RANDOM)
        face = np.where(i < N_FAR, i % min(len(v), 37), (7 * i) % len(v))
        aimed = (i < N_FAR) | (i % 4 != 0)
        o, length = random[:, 3:6].astype(np.float64), np.linalg.norm(random[:, 0:3].astype(np.float64), axis=1, keepdims=True)
        d = centroid[face] - o
        behind = (d * normal[face]).sum(axis=1) > 0
        o[behind] = 2.0 * centroid[face][behind] - o[behind]
        d[behind] = -d[behind]
        d *= length / np.linalg.norm(d, axis=1, keepdims=True)
        random[aimed, 0:3], random[aimed, 3:6] = d[aimed].astype(np.float32), o[aimed].astype(np.float32)
        parts = [random, QC.light_rays(rest, hs.lights, N_LIGHTS), QC.far_rays(random[:N_FAR]), QC.hostile_rays(rest, random[N_FAR:N_FAR + N_HOSTILE])]
        self.rays = np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)
        edges = np.cumsum([0] + [len(p) for p in parts])
        self.parts = {k: slice(int(edges[j]), int(edges[j + 1])) for j, k in enumerate(("random", "lights", "far", "hostile"))}
        with np.errstate(all="ignore"):
            want = O.intersect(O.OracleScene.from_host_scene(hs, P.cubemap_from_color()), self.rays)
        self.t_range = QC.ranges_for(rest, want)
        assert len(self.rays) == N_RAYS
        self.rays.setflags(write=False)
        self.t_range.setflags(write=False)

    def aimed_at(self, lights):
        """the ray array with its 64 light rays aimed at `lights` (after a lights op, so that they keep hitting lights)"""
        rays = self.rays.copy()
        rays[self.parts["lights"]] = QC.light_rays(np.random.default_rng(1083), lights, N_LIGHTS)    # (the origins and lengths of the start's)
        return rays


# ---------------------------------------------------------------- what the readers must answer, and the comparisons

_expected = {}


def expected(P, O, hs, rays, t_range, frame=True, key=None):
    """What every reader must answer for the descriptor `hs`: the oracle's frame, the query mirror's records, and what
    host_scene_tables states of tables 3 and 4 (the compact records behind table 4's general ones only while the scene is flat).
    key: (sequence index, step) of a caller that takes a Model along a sequence of sequences(): the model is a function of the two, so
    the answer is computed once per key and handed out again, its arrays read-only (a second run of the sequence, under other
    contents of fresh device memory, costs device time only)."""
    if key is not None and (key, frame) in _expected:
        return _expected[key, frame]
    out = _compute_expected(P, O, hs, rays, t_range, frame)
    if key is not None:
        for v in out.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _expected[key, frame] = out
    return out


def _compute_expected(P, O, hs, rays, t_range, frame):
    out = {}
    if frame:
        out["frame"] = O.render(O.OracleScene.from_host_scene(hs, P.cubemap_from_color()), O.camera_from_record(hs.camera), *SIZE, spp=SPP, bounces=BOUNCES)
    with np.errstate(all="ignore"):
        out["hits"], out["uv"] = P.host_query_rays(hs.faces, hs.lights, rays, t_range)
        out["occluded"] = P.host_query_rays(hs.faces, hs.lights, rays, t_range, mode="any")
    t = P.host_scene_tables(hs)
    n, flat = len(hs.faces), hs.is_flat()
    out["tris_brute"], out["shade"] = t["tris_brute"], t["shade"][: n * (112 + 64) if flat else n * 112]
    out["flat"], out["n_faces"], out["margins"] = flat, n, t["scalars"][:3].copy()
    return out


def mismatches(got, want):
    """The readers of `got` that do not answer as `want` does, bit for bit: a list of (reader, how many items differ)."""
    bad = []

    def differ(name, a, b):
        a, b = (np.ascontiguousarray(x).view(np.uint8).reshape(-1) for x in (a, b))
        if a.shape != b.shape:
            bad.append((name, -1))
        elif (a != b).any():
            bad.append((name, int((a != b).sum())))

    if "frame" in got and "frame" in want:
        differ("accumulator", got["frame"][0], want["frame"][0])
        differ("surface", got["frame"][1], want["frame"][1])
    for name in ("hits", "uv", "occluded", "tris_brute", "margins"):
        if name in got:
            differ(name, got[name], want[name])
    if "shade" in got:
        n = want["n_faces"] * (112 + (64 if want["flat"] else 0))
        differ("shade", got["shade"][:n], want["shade"][:n])
    for name in ("flat", "n_faces"):
        if name in got and got[name] != want[name]:
            bad.append((name, 1))
    return bad


def assert_answers(got, want, what):
    bad = mismatches(got, want)
    assert not bad, f"{what}: readers that do not answer for the scene of now: {bad}"


def pixel_share(a, b):
    """the share of a frame's pixels whose accumulator differs by a bit"""
    return float((a[0].view(np.uint32) != b[0].view(np.uint32)).any(axis=2).mean())


def ray_shares(a, b):
    """(share of rays whose record differs by a byte, rays whose kind or index differs)"""
    return float((a["hits"] != b["hits"]).any(axis=1).mean()), int((a["hits"][:, :2] != b["hits"][:, :2]).any(axis=1).sum())


def with_camera(P, hs, camera):
    return P.HostScene(hs.faces, hs.mesh_sizes, hs.materials, hs.lights, hs.textures, hs.texels, camera, hs.cubemap)


def steps(P, seq, ray_set):
    """The model taken along `seq`: yields (i, kind, call, the scene before, the scene after, the rays before, the rays after, model)
    per op; the light rays are aimed again after a lights op."""
    model = Model(P, seq.start, seq.mixed)
    rays = ray_set.rays
    for i, kind in enumerate(seq.kinds):
        before, rays_before = model.scene(), rays
        call = model.apply(kind)
        if kind == "lights":
            rays = ray_set.aimed_at(model.lights)
        yield i, kind, call, before, model.scene(), rays_before, rays, model
