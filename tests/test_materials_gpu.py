"""ptamd_scene_update_materials on the device (include/ptamd.h "Other materials, other texels"): one scene id taken through changes
of its material table, texture descriptors, texel blob and ids against a fresh upload's shading records and the oracle, with
everything the tree decides untouched; records that a refit, a rebuild or a pose has since rewritten; the asynchronous texel path
and its order on a stream; refusals that change nothing; what the other calls make of the new tables."""
import ctypes as C
import re

import numpy as np
import pytest

from materials_cases import BLOB, COUNTS, changed, states, with_material
from replace_cases import faces_tensor, material_scene, mirror, mixed_ids, replaced
from test_gpu_parity import assert_same
from test_rebuild_gpu import assert_tables, group_prims, oracle
from test_refit_device_gpu import device_faces, same_bits
from test_refit_gpu import B, KINDS, render

pytestmark = pytest.mark.gpu

SIZE = (64, 48)
FLAT_FORMS = (8, 9, 11, 14)   # PT_RS_FLAT, _FLAT_SKIP, _FLAT_SKIP_DEFER, _FLAT_SKIP_TIGHT (csrc/pt_device.h)
TREE_TABLES = ("nodes", "tris_bvh", "nodes4", "tris_brute")


@pytest.fixture(scope="module")
def gpu_ctx(P):
    """A context of this module's own (an update is refused while any stream of its context holds a captured launch)."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback for the render path")
    ctx = P.Context(0)
    yield ctx
    errors = ctx.device_error_count()
    ctx.close()
    assert errors == 0


def ids_tensor(ids):
    import torch
    return torch.from_numpy(np.ascontiguousarray(ids, np.uint32).view(np.int32).copy()).cuda()


def apply(ctx, sid, step, stream=None):
    """A step of materials_cases as the call takes it: a whole new blob comes with its new size"""
    kw = dict(materials=step.get("materials"), textures=step.get("textures"), stream=stream)
    if "texels" in step:
        kw.update(texels=step["texels"], n_texel_floats=len(step["texels"]))
    if "ids" in step:
        kw.update(material_ids=ids_tensor(step["ids"]))
    return ctx.update_scene_materials(sid, **kw)


def tree_state(ctx, sid):
    """Everything the call must leave as it is"""
    t = ctx.read_scene_tables(sid)
    return dict(tables={k: t[k] for k in TREE_TABLES}, links=ctx.scene_links(sid), plan=ctx.read_scene_plan(sid), margins=ctx.scene_margins(sid),
                quality=ctx.scene_quality(sid), info=ctx.scene_info(sid))


def assert_tree_state(ctx, sid, before, what):
    now = tree_state(ctx, sid)
    for k in TREE_TABLES:
        np.testing.assert_array_equal(now["tables"][k], before["tables"][k], err_msg=f"{what}: table {k} changed")
    np.testing.assert_array_equal(now["links"], before["links"], err_msg=what + ": the link table changed")
    assert now["plan"]["counts"] == before["plan"]["counts"], what
    for name in ("refit_groups", "refit_levels", "refit_sched", "wide_child"):
        np.testing.assert_array_equal(now["plan"][name], before["plan"][name], err_msg=f"{what}: plan table {name} changed")
    same_bits(now["margins"], before["margins"], what + ": margins")
    assert now["quality"] == before["quality"] and now["info"] == before["info"], what


def flat_state(P, ctx, ids, cam):
    """(ptamd_scene_is_flat, the restart kernel took a flat form, table 4 has the compact tail)"""
    sid, cid = ids
    render(P, ctx, ids, cam, P.KERNEL_BVH_RESTART, size=SIZE)
    n = ctx.scene_info(sid)["n_faces"]
    return ctx.scene_is_flat(sid, cid), ctx.last_restart_form() in FLAT_FORMS, ctx.read_scene_tables(sid)["shade"].size == n * (112 + 64)


# ---------------------------------------------------------------- 1. the tables path

@pytest.mark.parametrize("n", COUNTS)
def test_tables_ids_and_blob_change_on_one_scene_id(P, O, gpu_ctx, n):
    """The transitions of materials_cases in sequence.  After each: table 4 is a fresh upload's of the changed descriptor (size
    included), everything the tree decides is byte-identical to what it was, flatness and the launch form follow, the info reports
    both flatnesses, and every kernel kind renders the oracle's frame of the new descriptor."""
    cube = P.cubemap_from_color()
    start = material_scene(P, n)
    cam = start.camera_struct()
    sid, cid = gpu_ctx.upload_scene(start), gpu_ctx.upload_cubemap(cube)
    # (500 faces lie beyond the compact layout: their launches take the walk from L2, which has no flat form)
    si = gpu_ctx.scene_info(sid)
    resident = si["lds_bytes_bvh"] <= 64 * 1024 and si["n_nodes"] <= 896
    assert resident == (n != 500), si
    assert flat_state(P, gpu_ctx, (sid, cid), cam) == (True, resident, True)
    for what, step, old, new in states(P, n):
        what = f"n = {n}, {what}"
        before = tree_state(gpu_ctx, sid)
        info = apply(gpu_ctx, sid, step)
        flat = new.is_flat()
        assert info == dict(flat_before=int(old.is_flat()), flat=int(flat), asynchronous=0, reserved=0), (what, info)
        want = P.host_scene_tables(new)["shade"]
        got = gpu_ctx.read_scene_tables(sid)["shade"]
        assert got.size == want.size == n * (112 + (64 if flat else 0)), (what, got.size, want.size)
        np.testing.assert_array_equal(got, want, err_msg=what + ": table 4 against a fresh upload's")
        assert_tree_state(gpu_ctx, sid, before, what)
        assert flat_state(P, gpu_ctx, (sid, cid), cam) == (flat, flat and resident, flat), (what, flat_state(P, gpu_ctx, (sid, cid), cam))
        ref = oracle(O, new, cube, SIZE, spp=2, bounces=B)
        for kind in KINDS:
            assert_same(*render(P, gpu_ctx, (sid, cid), cam, getattr(P, kind), size=SIZE), *ref, f"{what}: {kind} vs oracle")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 2. records that geometry has since rewritten

def test_records_a_refit_has_rewritten_and_the_refits_that_follow(P, O, gpu_ctx):
    import rig_cases as RC
    n = 300
    cube = P.cubemap_from_color()
    start = material_scene(P, n)
    sid, cid = gpu_ctx.upload_scene(start), gpu_ctx.upload_cubemap(cube)
    moved = P.deform(start, 0.7, 0.05, shading=True)
    gpu_ctx.update_scene_device(sid, device_faces(moved))
    mixed, plain = changed(P, start, ids=mixed_ids(n)), start
    for what, new in (("to mixed ids", mixed), ("to all m0", plain)):
        before = tree_state(gpu_ctx, sid)
        info = gpu_ctx.update_scene_materials(sid, material_ids=ids_tensor(new.faces["material_id"]))
        assert info["flat"] == int(new.is_flat()), (what, info)
        np.testing.assert_array_equal(gpu_ctx.read_scene_tables(sid)["shade"], P.host_scene_tables(new, moved)["shade"], err_msg=what + ", moved faces")
        assert_tree_state(gpu_ctx, sid, before, what)
        ref = oracle(O, changed(P, moved, ids=new.faces["material_id"]), cube, SIZE, spp=2, bounces=B)
        assert_same(*render(P, gpu_ctx, (sid, cid), start.camera_struct(), P.KERNEL_AUTO, size=SIZE), *ref, what + ", moved faces: default kernel vs oracle")
    # flat again: the compact normals are those of the moved faces (the tail the non-flat scene had was stale), and follow the next ones
    assert gpu_ctx.scene_is_flat(sid, cid)
    for new in (mixed, plain):
        gpu_ctx.update_scene_materials(sid, material_ids=ids_tensor(new.faces["material_id"]))
        again = P.deform(start, 1.9, 0.04, shading=True)
        gpu_ctx.update_scene_device(sid, device_faces(again))
        np.testing.assert_array_equal(gpu_ctx.read_scene_tables(sid)["shade"], P.host_scene_tables(new, again)["shade"], err_msg="a refit behind the update")
        sizes = [n // 2, n - n // 2]
        with gpu_ctx.scene_rig(sid, new, sizes) as rig:
            t, m = RC.matrices(2, 8, RC.extent_of(new), "rigid")
            rig.pose(t, m)
            posed = P.host_pose_faces(new, t, m, sizes)
            got, want = gpu_ctx.read_scene_tables(sid), P.host_scene_tables(new, posed)
            for name in ("tris_brute", "shade"):
                np.testing.assert_array_equal(got[name], want[name], err_msg=name + " after a pose behind the update")
    gpu_ctx.release_scene(sid)


@pytest.mark.parametrize("finish", [False, True])
def test_records_a_rebuild_has_rewritten(P, O, gpu_ctx, finish):
    n = group_prims(P) + 200
    cube = P.cubemap_from_color()
    start = material_scene(P, n)
    sid, cid = gpu_ctx.upload_scene(start), gpu_ctx.upload_cubemap(cube)
    moved = P.deform(start, 0.7, 0.05, shading=True)
    assert gpu_ctx.rebuild_scene_device(sid, device_faces(moved), device_finish=finish)["device_builder"] == (2 if finish else 1)
    new = changed(P, start, ids=mixed_ids(n))
    before = tree_state(gpu_ctx, sid)
    info = gpu_ctx.update_scene_materials(sid, material_ids=ids_tensor(new.faces["material_id"]))
    assert info == dict(flat_before=1, flat=0, asynchronous=0, reserved=0)
    want = P.host_rebuild_tables(new, moved)
    assert_tables(gpu_ctx.read_scene_tables(sid), want, "the update behind a rebuild")
    assert_tree_state(gpu_ctx, sid, before, "the update behind a rebuild")
    ref = oracle(O, changed(P, moved, ids=new.faces["material_id"]), cube, SIZE, spp=2, bounces=B)
    for kind in ("KERNEL_BVH", "KERNEL_BVH_RESTART", "KERNEL_BRUTE_FORCE"):
        assert_same(*render(P, gpu_ctx, (sid, cid), start.camera_struct(), getattr(P, kind), size=SIZE), *ref, f"behind a rebuild: {kind} vs oracle")
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 3. the texel path

def texel_cases():
    rng = np.random.default_rng(31)
    new = lambda k: rng.uniform(0.05, 0.95, size=k).astype(np.float32)
    return [("m0's 1x1 texel, from the host", 0, new(4), False), ("m0's 1x1 texel, from the device", 0, new(4), True),
            ("a sub-range of the 4x4 map", 8 + 5, new(7), False), ("both 1x1 texels and the map's head, from the device", 0, new(12), True),
            ("a range that ends at the blob's last float", BLOB - 6, new(6), False), ("no float at all", 17, new(0), False)]


@pytest.mark.parametrize("flat", [False, True])
def test_texel_ranges_alone(P, O, gpu_ctx, flat):
    """On a scene with every kind of material and on a flat one (whose compact records carry the texel too).  Table 4 and the frame
    equal a fresh upload's and the oracle's of the descriptor with the range substituted; the call reports the asynchronous path."""
    import torch
    n = 300
    cube = P.cubemap_from_color()
    hs = material_scene(P, n, None if flat else mixed_ids(n))
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    before = tree_state(gpu_ctx, sid)
    for what, first, values, device in texel_cases():
        blob = hs.texels.copy()
        blob[first:first + len(values)] = values
        hs = changed(P, hs, texels=blob)
        src = torch.from_numpy(values.copy()).cuda() if device else values
        info = gpu_ctx.update_scene_materials(sid, texels=src, texel_first=first)
        assert info == dict(flat_before=int(flat), flat=int(flat), asynchronous=1, reserved=0), (what, info)
        np.testing.assert_array_equal(gpu_ctx.read_scene_tables(sid)["shade"], P.host_scene_tables(hs)["shade"], err_msg=what)
        ref = oracle(O, hs, cube, SIZE, spp=2, bounces=B)
        for kind in ("KERNEL_BVH_RESTART", "KERNEL_BVH", "KERNEL_BRUTE_FORCE"):
            assert_same(*render(P, gpu_ctx, (sid, cid), hs.camera_struct(), getattr(P, kind), size=SIZE), *ref, f"{what}: {kind} vs oracle")
        assert flat_state(P, gpu_ctx, (sid, cid), hs.camera_struct()) == (flat, flat, flat), what
    assert_tree_state(gpu_ctx, sid, before, "the texel path")
    gpu_ctx.release_scene(sid)


def test_texel_updates_are_ordered_on_their_stream(P, O, gpu_ctx):
    """render, update, render, update (device range), render on one stream with no host wait between them: each frame is the
    oracle's of the descriptor of its time."""
    import torch
    n = 300
    cube = P.cubemap_from_color()
    a = material_scene(P, n, mixed_ids(n))
    blob_b, blob_c = a.texels.copy(), a.texels.copy()
    blob_b[0:4] = (0.1, 0.9, 0.2, 0.4)
    blob_c[0:4] = blob_b[0:4]
    blob_c[4:8] = (0.9, 0.1, 0.6, 0.2)
    b, c = changed(P, a, texels=blob_b), changed(P, a, texels=blob_c)
    sid, cid = gpu_ctx.upload_scene(a), gpu_ctx.upload_cubemap(cube)
    cam = a.camera_struct()
    frames = [P.FrameRenderer(gpu_ctx, sid, cid, cam, *SIZE) for _ in range(3)]
    second = torch.from_numpy(blob_c[4:8].copy()).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, stream=side, fr=frames[0], spp=2, size=SIZE)
        gpu_ctx.update_scene_materials(sid, texels=blob_b[0:4], texel_first=0, stream=side)
        render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, stream=side, fr=frames[1], spp=2, size=SIZE)
        gpu_ctx.update_scene_materials(sid, texels=second, texel_first=4, stream=side)
        render(P, gpu_ctx, (sid, cid), cam, P.KERNEL_AUTO, stream=side, fr=frames[2], spp=2, size=SIZE)
    torch.cuda.synchronize()
    for fr, hs, what in zip(frames, (a, b, c), ("before the updates", "behind the first", "behind the second")):
        assert_same(fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), *oracle(O, hs, cube, SIZE, spp=2, bounces=B), "the frame " + what)
    np.testing.assert_array_equal(gpu_ctx.read_scene_tables(sid)["shade"], P.host_scene_tables(c)["shade"])
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 4. refusals

def test_refusals_leave_everything_as_it_was(P):
    """Every case is refused on the host, or by the id check before anything is moved: no kernel is launched with a bad pointer."""
    import torch
    N = P.native
    n = 300
    cube = P.cubemap_from_color()
    start = material_scene(P, n, mixed_ids(n))
    cam = start.camera_struct()
    with P.Context(0) as ctx:
        lib = ctx._lib
        cid = ctx.upload_cubemap(cube)
        sid, gone = ctx.upload_scene(start), ctx.upload_scene(start)
        ctx.release_scene(gone)
        ctx.update_scene(sid, start)      # (every refusal below is followed by this update: the state it leaves is the one compared)
        keep = render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO, size=SIZE)
        state, shade, flat = tree_state(ctx, sid), ctx.read_scene_tables(sid)["shade"], ctx.scene_is_flat(sid, cid)

        def refused(call, status, word):
            with pytest.raises(P.PtamdError) as err:
                call()
            assert err.value.status == status and word in str(err.value), str(err.value)
            np.testing.assert_array_equal(ctx.read_scene_tables(sid)["shade"], shade, err_msg="table 4 after the refusal: " + word)
            assert_tree_state(ctx, sid, state, "after the refusal: " + word)
            assert ctx.scene_is_flat(sid, cid) == flat
            assert_same(*render(P, ctx, (sid, cid), cam, P.KERNEL_AUTO, size=SIZE), *keep, "after the refusal: " + word)
            ctx.update_scene(sid, start)     # the accepted ids are the old ones
            return str(err.value)

        def raw(scene=sid, materials=None, n_materials=0, textures=None, n_textures=0, texels=None, first=0, count=0, size=0, ids=None, flags=0):
            d = N.SceneMaterialsDesc()
            d.scene_id, d.materials, d.n_materials, d.textures, d.n_textures = scene, materials, n_materials, textures, n_textures
            d.texels, d.texel_first, d.texel_count, d.n_texel_floats, d.material_ids, d.flags = texels, first, count, size, ids, flags
            N.check(lib.ptamd_scene_update_materials(ctx._h, C.byref(d), None))

        ARG, update = N.PTAMD_ERR_ARG, ctx.update_scene_materials
        # a bad id, found on the device before anything is moved: the lowest face is named
        ids = mixed_ids(n)
        ids[[200, 17, 299]] = 3
        text = refused(lambda: update(sid, material_ids=ids_tensor(ids)), ARG, "material_id")
        assert re.search(r"\bface 17\b", text), text
        ids = mixed_ids(n)
        ids[n - 1] = 0xFFFFFFFF
        text = refused(lambda: update(sid, material_ids=ids_tensor(ids), materials=start.materials), ARG, "material_id")
        assert re.search(r"\bface %d\b" % (n - 1), text), text
        # kept ids under a smaller table, checked on the host
        refused(lambda: update(sid, materials=start.materials[:1]), ARG, "material_id")
        # tables the upload would refuse
        past = start.textures.copy()
        past["offset"][3] = BLOB - 47
        refused(lambda: update(sid, textures=past), ARG, "out of the texel blob")
        refused(lambda: update(sid, texels=start.texels[:100], n_texel_floats=100), ARG, "out of the texel blob")   # (the kept tables, a shorter blob)
        refused(lambda: update(sid, materials=with_material(P, start, 0, diffuse_spec_map=3)), ARG, "4-channel")
        refused(lambda: update(sid, materials=with_material(P, start, 1, normal_map=4)), ARG, "texture id invalid")
        # ranges
        four = np.zeros(4, np.float32)
        refused(lambda: update(sid, texels=four, texel_first=BLOB - 3), ARG, "outside the blob")
        refused(lambda: update(sid, texels=four, texel_first=1 << 40), ARG, "outside the blob")
        refused(lambda: update(sid, texels=four, n_texel_floats=BLOB), ARG, "new size")
        refused(lambda: update(sid, texels=four, texel_first=2, n_texel_floats=4), ARG, "new size")
        refused(lambda: raw(size=BLOB), ARG, "new size")
        refused(lambda: raw(texels=four.ctypes.data, count=4, size=1 << 32), N.PTAMD_ERR_LIMIT, "2^32")
        # pointers: refused before anything reads them
        roomy = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
        refused(lambda: raw(ids=roomy.data_ptr() + 4), ARG, "16 bytes")
        refused(lambda: raw(texels=roomy.data_ptr() + 4, count=4, flags=1), ARG, "16 bytes")
        host_ids = np.zeros(n + 4, np.uint32)
        aligned = (host_ids.ctypes.data + 15) & ~15
        refused(lambda: raw(ids=aligned), ARG, "not device memory")
        refused(lambda: raw(texels=aligned, count=4, flags=1), ARG, "not device memory")
        exact = C.c_void_p()
        N.check(lib.ptamd_device_alloc(ctx._h, 64 * 4, C.byref(exact)))
        try:
            refused(lambda: raw(ids=exact.value), ARG, "smaller than the call reads")
        finally:
            N.check(lib.ptamd_device_free(ctx._h, exact))
        # the descriptor's shape
        refused(lambda: raw(flags=2), ARG, "unknown flag")
        refused(lambda: raw(flags=0x80000001), ARG, "unknown flag")
        mats = np.ascontiguousarray(start.materials)
        refused(lambda: raw(n_materials=3), ARG, "count without its table")
        refused(lambda: raw(materials=mats.ctypes.data_as(C.POINTER(N.Material))), ARG, "count without its table")
        refused(lambda: raw(n_textures=4), ARG, "count without its table")
        refused(lambda: update(gone, texels=four), ARG, "released")
        refused(lambda: update(99, texels=four), ARG, "out of range")
        for bad in (roomy.cpu(), roomy[:n].view(torch.int16), roomy[:n - 1]):
            with pytest.raises(ValueError):
                update(sid, material_ids=bad)
        # a capturing stream cannot hold an update
        side = torch.cuda.Stream()
        dummy = torch.zeros(64, device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dummy.add_(1.0)
            with pytest.raises(P.PtamdError) as err:
                update(sid, texels=four, stream=torch.cuda.current_stream())
        assert err.value.status == N.PTAMD_ERR_LIMIT and "captured into a graph" in str(err.value)
        del g
        torch.cuda.synchronize()
        # ... and a call that was refused goes through afterwards
        info = update(sid, materials=start.materials[:1], material_ids=ids_tensor(np.zeros(n, np.uint32)))
        assert info["flat"] == 1 and ctx.scene_is_flat(sid, cid)
        assert ctx.device_error_count() == 0


# ---------------------------------------------------------------- 5. what follows

def test_what_follows_an_update(P, O, gpu_ctx):
    import rig_cases as RC
    n = 300
    cube = P.cubemap_from_color()
    old = material_scene(P, n)
    sid, cid = gpu_ctx.upload_scene(old), gpu_ctx.upload_cubemap(cube)
    sizes = [n // 2, n - n // 2]
    rig = gpu_ctx.scene_rig(sid, old, sizes)
    materials = with_material(P, old, 1, diffuse_spec_map=2, ior=1.0)
    new = changed(P, old, materials=materials, ids=mixed_ids(n))
    gpu_ctx.update_scene_materials(sid, materials=materials, material_ids=ids_tensor(mixed_ids(n)))
    # ptamd_scene_update takes faces with the new ids and refuses the old ones
    moved = P.deform(new, 0.7, 0.05, shading=True)
    gpu_ctx.update_scene(sid, moved)
    np.testing.assert_array_equal(gpu_ctx.read_scene_tables(sid)["shade"], P.host_scene_tables(new, moved)["shade"])
    with pytest.raises(P.PtamdError) as err:
        gpu_ctx.update_scene(sid, old)
    assert err.value.status == P.native.PTAMD_ERR_ARG and "material_id" in str(err.value)
    # a rig made before the call still poses: positions from the rig, material words from the scene
    t, m = RC.matrices(2, 8, RC.extent_of(old), "rigid")
    rig.pose(t, m)
    posed = P.host_pose_faces(new, t, m, sizes)
    got, want = gpu_ctx.read_scene_tables(sid), P.host_scene_tables(new, posed)
    for name in ("tris_brute", "shade"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=name + " after the pose of a rig made before the update")
    ref = oracle(O, posed, cube, SIZE, spp=2, bounces=B)
    assert_same(*render(P, gpu_ctx, (sid, cid), old.camera_struct(), P.KERNEL_AUTO, size=SIZE), *ref, "the posed scene vs oracle")
    rig.close()
    # ptamd_scene_replace forms its words from the new tables
    grown = replaced(P, new, changed(P, material_scene(P, 420, mixed_ids(420), seed=6), materials=materials))
    info = gpu_ctx.replace_scene_faces(sid, faces_tensor(grown))
    compact = gpu_ctx.scene_info(sid)["lds_bytes_bvh"] <= 64 * 1024 and info["n_nodes"] <= 896
    assert_tables(gpu_ctx.read_scene_tables(sid), mirror(P, grown, compact), "a replace behind the update")
    ref = oracle(O, grown, cube, SIZE, spp=2, bounces=B)
    assert_same(*render(P, gpu_ctx, (sid, cid), grown.camera_struct(), P.KERNEL_AUTO, size=SIZE), *ref, "the replaced scene vs oracle")
    gpu_ctx.release_scene(sid)


def test_the_motion_denoiser_keeps_its_history(P, gpu_ctx):
    """No face moves and none becomes another: neither serial of the scene moves, the denoiser's snapshot stays the one it took, and
    the history is not cut."""
    import test_denoise_motion_gpu as DM
    W, H = 96, 54
    hs, cube = DM.wide(P)
    sid, cid = gpu_ctx.upload_scene(hs), gpu_ctx.upload_cubemap(cube)
    cam0 = hs.camera_struct()
    fr = P.FrameRenderer(gpu_ctx, sid, cid, cam0, W, H)
    with gpu_ctx.denoise_history(W, H) as ha:
        for k in range(2):
            fr.cam = P.orbit_camera(cam0, DM.STEP * k)
            fr.render(spp=4, reset=True)
            a = DM.denoise(fr, ha)
        assert a[2].max() == 2.0 and (a[2] > 1).mean() > 0.3
        before = ha.read_geometry()
        gpu_ctx.update_scene_materials(sid, materials=hs.materials, material_ids=ids_tensor(hs.faces["material_id"]))
        gpu_ctx.update_scene_materials(sid, texels=hs.texels[:4], texel_first=0)
        fr.cam = P.orbit_camera(cam0, DM.STEP * 2)
        fr.render(spp=4, reset=True)
        a = DM.denoise(fr, ha)
        after = ha.read_geometry()
        assert (after["scene_id"], after["serial"]) == (before["scene_id"], before["serial"]) and np.array_equal(after["tris"], before["tris"])
        assert (a[2] > 1).mean() > 0.3, "the history was cut"
    gpu_ctx.release_scene(sid)


# ---------------------------------------------------------------- 6. registers

def test_the_rematerial_kernel_has_no_scratch():
    """csrc/pt_rematerial.hip by the recipe of test_reface_kernels_have_no_scratch: no private segment, no spilled register, the
    2 KB of LDS its head states."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_listing
    if kernel_listing.hipcc() is None:
        pytest.skip("no hipcc on this host")
    text = kernel_listing.listing("pt_rematerial.hip")
    meta = kernel_listing.all_metadata(text)
    assert len(meta) == 1 and "pt_rematerial_faces" in next(iter(meta)), sorted(meta)
    for name, m in meta.items():
        print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", text) == ["2048"]
