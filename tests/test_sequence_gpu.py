"""One scene id through long, mixed sequences of the calls that change an uploaded scene, every reader held to the oracle or to its
host mirror after EVERY op (tests/sequence_cases.py: the model, the sequences and the comparisons; tests/test_sequence_cpu.py: what
this rests on; DESIGN.md §13 "Sequences").

Whatever the history of a scene id, every reader answers for the descriptor the scene holds now: frames against the CPU oracle bit
for bit (48 x 48, 2 spp, 3 bounces), ray queries of every walk the scene allows and both modes against ptamd_host_query_rays byte for
byte, tables 3 and 4, flatness, the face count, margins, the cull count and (after a relink) the link table against the host
mirrors, the adaptive list form against the uniform frame.  The first two sequences run a second time with ops and readers enqueued
on one side stream and no host wait between an op and the readers behind it.  No tolerance anywhere."""
import numpy as np
import pytest

import sequence_cases as S
from test_gpu_parity import assert_same
from test_query_gpu import same
from test_refit_gpu import KINDS, render

pytestmark = pytest.mark.gpu

SEQUENCES = S.sequences()
FORM_BRUTE = 3          # PT_RS_BRUTE (csrc/pt_device.h): a camera or a light beyond the margins' reach
BUILDER = {"upload": None, "host": 0, "device": 1, "device_finish": 2}      # ptamd_scene_rebuild_info.device_builder
_results, _rays = {}, {}


@pytest.fixture(scope="module")
def gpu_ctx(P):
    """A context of this module's own (updates are refused while a captured launch pins the shared one)."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU; there is no CPU fallback for the render path")
    ctx = P.Context(0)
    yield ctx
    errors = ctx.device_error_count()
    ctx.close()
    assert errors == 0


def rays_of(P, O, start):
    if start not in _rays:
        _rays[start] = S.Rays(P, O, S.start_scene(P, start))
    return _rays[start]


def faces_tensor(hs):
    import torch
    return torch.from_numpy(np.ascontiguousarray(hs.faces).view(np.uint8).reshape(len(hs.faces), 112).copy()).cuda()


class Device:
    """The scene id of one sequence, its rig, and the device calls of the model's ops."""

    def __init__(self, P, ctx, model, stream=None):
        self.P, self.ctx, self.stream = P, ctx, stream
        self.sid, self.cid = ctx.upload_scene(model.scene()), ctx.upload_cubemap(P.cubemap_from_color())
        self.keep = []      # device arrays the calls read in stream order
        self.rig = None
        r = model.rig
        self.open_rig(model.scene(r["rest"]), r["sizes"], r["skin"], r["targets"])

    def open_rig(self, rest, sizes, skin, targets):
        """a rig with its skin and morph targets attached at once, so that a later refusal is the count's and nothing else's"""
        if self.rig is not None:
            self.rig.close()
        self.rig = self.ctx.scene_rig(self.sid, rest, sizes)
        self.rig.attach_skin(*skin)
        self.rig.attach_morphs(targets)

    def rig_call(self, call, refused=False):
        if call["kind"] == "pose":
            self.rig.pose(call["refused_transforms" if refused else "transforms"], None, stream=self.stream)
        elif call["kind"] == "skin":
            self.rig.skin(call["transforms"], None, stream=self.stream)
        else:
            self.rig.morph(call["weights"], stream=self.stream)

    def apply(self, call, model):
        """the device call of one op; returns ptamd_scene_rebuild_info of a rebuild or a replace"""
        import torch
        P, ctx, sid, st, kind = self.P, self.ctx, self.sid, self.stream, call["kind"]
        if kind == "update_host":
            ctx.update_scene(sid, call["scene"], stream=st)
        elif kind == "update_device":
            self.keep.append(faces_tensor(call["scene"]))
            ctx.update_scene_device(sid, self.keep[-1], stream=st)
        elif kind in ("rebuild", "rebuild_finish"):
            self.keep.append(faces_tensor(call["scene"]))
            return ctx.rebuild_scene_device(sid, self.keep[-1], stream=st, device_finish=call["finish"])
        elif kind in ("replace", "replace_finish"):
            self.keep.append(faces_tensor(call["scene"]))
            return ctx.replace_scene_faces(sid, self.keep[-1], stream=st, device_finish=call["finish"])
        elif kind == "materials":
            ids = None
            if "ids" in call:
                ids = torch.from_numpy(call["ids"].astype(np.uint32).view(np.int32).copy()).cuda()
                self.keep.append(ids)
            info = ctx.update_scene_materials(sid, materials=call.get("materials"), material_ids=ids, stream=st)
            assert info["asynchronous"] == 0 and bool(info["flat"]) == model.scene().is_flat(), info
        elif kind == "texels":
            src = call["values"]
            if call["device"]:
                src = torch.from_numpy(src.copy()).cuda()
                self.keep.append(src)
            info = ctx.update_scene_materials(sid, texels=src, texel_first=call["first"], stream=st)
            assert info["asynchronous"] == 1 and info["flat"] == info["flat_before"], info
        elif kind in S.RIG:
            if call["rig"] == "refused":
                # the rig is of the count before the last replace (sequence_cases.FORBIDDEN): refused with nothing changed, then reopened
                with pytest.raises(P.PtamdError) as err:
                    self.rig_call(call, refused=True)
                assert err.value.status == P.native.PTAMD_ERR_ARG and "n_faces" in str(err.value), str(err.value)
                assert ctx.scene_info(sid)["n_faces"] == len(call["rest"].faces)
                self.open_rig(call["rest"], call["sizes"], call["skin"], call["targets"])
            self.rig_call(call)
        elif kind == "lights":
            ctx.update_lights(sid, call["lights"], stream=st)
        else:
            assert kind == "relink"
            ctx.relink_scene(sid, stream=st)
        return None

    def allows(self):
        """the walks the scene allows NOW (include/ptamd.h): it changes across a replace"""
        si = self.ctx.scene_info(self.sid)
        allowed = ["auto", "every_face", "binary"] + (["wide"] if si["n_nodes4"] != 0 else [])
        resident = si["lds_bytes_bvh"] <= 65536 and si["n_nodes"] <= 896
        return allowed + (["resident"] if resident else []), resident, si

    def close(self):
        self.rig.close()
        self.ctx.release_scene(self.sid)


def kinds_after(step, last, changed):
    """KERNEL_AUTO and one other kind in rotation; every kind after the last op and after an op that changed the builder's path or
    the layout"""
    return ("KERNEL_AUTO",) + (KINDS if last or changed else (KINDS[step % len(KINDS)],))


def adaptive_list_form(P, ctx, dev, hs, far, want, what):
    """render_adaptive(st, 2, 2, 2, rounds=1, threshold=0.0): every pixel on the list once; accumulator and surface equal the uniform
    2-spp frame already held to the oracle.  Beyond the margins' reach the list form is refused (include/ptamd.h)."""
    import torch
    fr = P.FrameRenderer(ctx, dev.sid, dev.cid, hs.camera_struct(), *S.SIZE)
    with ctx.adaptive_state(*S.SIZE) as st:
        if far:
            with pytest.raises(P.PtamdError) as err:
                fr.render_adaptive(st, 2, 2, 2, rounds=1, threshold=0.0, bounces=S.BOUNCES, stream=dev.stream)
            assert err.value.status == P.native.PTAMD_ERR_ARG and "beyond the reach" in str(err.value), str(err.value)
            return False
        fr.render_adaptive(st, 2, 2, 2, rounds=1, threshold=0.0, bounces=S.BOUNCES, stream=dev.stream)
        torch.cuda.synchronize()
        assert (st.read()["counts"] == 2).all(), what
    assert_same(fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), *want["frame"], what + ": the adaptive list form")
    return True


def run_sequence(P, O, ctx, index):
    """Uploads the start scene once, applies the ops in order and checks every reader after every op.  Returns what the coverage
    asserts need: the restart forms seen and the kinds the resident walk ran behind."""
    import torch
    seq = SEQUENCES[index]
    rs = rays_of(P, O, seq.start)
    model = S.Model(P, seq.start, seq.mixed)
    dev = Device(P, ctx, model)
    t_range = torch.from_numpy(rs.t_range.copy()).cuda()
    rays_np, rays = rs.rays, torch.from_numpy(rs.rays.copy()).cuda()
    seen = dict(forms=[], resident_walk=set(), adaptive=0)
    _, was_resident, _ = dev.allows()
    assert was_resident == model.layout()["resident"], (seq, "the uploaded layout")
    was_how = None
    for step, kind in enumerate(seq.kinds):
        what = f"{seq} step {step} ({kind})"
        call = model.apply(kind)
        info = dev.apply(call, model)
        if kind == "lights":
            rays_np = rs.aimed_at(model.lights)
            rays = torch.from_numpy(rays_np).cuda()
        hs, lay = model.scene(), model.layout()
        want = S.expected(P, O, hs, rays_np, rs.t_range, key=(index, step))
        walks, resident, si = dev.allows()
        assert resident == lay["resident"], (what, si, lay)
        if info is not None:
            assert info["device_builder"] == BUILDER[lay["how"]], (what, info, lay)
        # ---- frames against the oracle
        changed = info is not None and (resident != was_resident or lay["how"] != was_how)
        has_links = ctx.scene_links(dev.sid).shape[0] > 0
        assert has_links == lay["links"], (what, "a link table", has_links, lay)
        for name in kinds_after(step, step == len(seq.kinds) - 1, changed):
            got = render(P, ctx, (dev.sid, dev.cid), hs.camera_struct(), getattr(P, name), size=S.SIZE)
            assert_same(*got, *want["frame"], f"{what}: {name} vs the oracle")
            form = ctx.last_restart_form()
            if form >= 0:
                assert (form == FORM_BRUTE) == model.far, (what, name, form)
                seen["forms"].append((form, kind, resident, has_links))
        # ---- ray queries against the mirror: every walk the scene allows now, both modes, with ranges
        for walk in walks:
            hits, uv = ctx.query_rays(dev.sid, rays, t_range, mode="nearest", walk=walk)
            occ = ctx.query_rays(dev.sid, rays, t_range, mode="any", walk=walk)
            torch.cuda.synchronize()
            same(hits, want["hits"], f"{what}: walk {walk} hits")
            same(uv, want["uv"], f"{what}: walk {walk} uv")
            same(occ.view(torch.uint8), want["occluded"], f"{what}: walk {walk} occluded")
            if walk == "resident":
                seen["resident_walk"].add(kind)
                if kind.startswith("replace") and not was_resident:
                    seen["resident_walk"].add("a replace that made the scene resident")
        # ---- what the model can state of the tables
        tables = ctx.read_scene_tables(dev.sid)
        margins = ctx.scene_margins(dev.sid)
        got = dict(tris_brute=tables["tris_brute"], shade=tables["shade"], flat=ctx.scene_is_flat(dev.sid, dev.cid), n_faces=si["n_faces"], margins=margins[:3])
        S.assert_answers(got, want, what)
        assert margins[3] == 1.0, what
        assert ctx.scene_cull_count(dev.sid) == model.expected_cull(), (what, ctx.scene_cull_count(dev.sid), model.expected_cull(), model.culled)
        if kind == "relink" and has_links:
            np.testing.assert_array_equal(ctx.scene_links(dev.sid), model.expected_links(), err_msg=what + ": the link table against ptamd_host_relink_words")
        # ---- the adaptive list form, after the op in the middle and after the last
        if step in (len(seq.kinds) // 2, len(seq.kinds) - 1):
            seen["adaptive"] += adaptive_list_form(P, ctx, dev, hs, model.far, want, what)
        was_resident, was_how = resident, lay["how"]
    assert ctx.device_error_count() == 0, seq
    # the id is released; a fresh upload under the same context renders the oracle's frame
    dev.close()
    fresh = ctx.upload_scene(hs)
    assert_same(*render(P, ctx, (fresh, dev.cid), hs.camera_struct(), P.KERNEL_AUTO, size=S.SIZE), *want["frame"], f"{seq}: a fresh upload afterwards")
    ctx.release_scene(fresh)
    return seen


def result_of(P, O, ctx, index):
    if index not in _results:
        _results[index] = run_sequence(P, O, ctx, index)
    return _results[index]


@pytest.mark.parametrize("index", range(len(SEQUENCES)))
def test_every_reader_after_every_op(P, O, gpu_ctx, index):
    result_of(P, O, gpu_ctx, index)


def test_the_forms_and_the_resident_walk_were_all_seen(P, O, gpu_ctx):
    """Over all sequences (run here where the cases above have not): a flat skip form, the plain skip form, a form over a scene that
    is not resident and one over a scene with no link table were each launched directly behind a device-side op; the resident
    query walk ran behind an update from device faces, a rebuild, a pose, a lights update, a relink and a replace that made the
    scene resident; the adaptive list form ran."""
    seen = [result_of(P, O, gpu_ctx, i) for i in range(len(SEQUENCES))]
    forms = [f for s in seen for f in s["forms"] if f[1] in S.DEVICE_SIDE]
    print("restart forms behind device-side ops:", sorted({(form, kind) for form, kind, _, _ in forms}))
    assert any(form == P.FORM_FLAT_SKIP for form, _, _, _ in forms), "a flat skip form"
    assert any(form == P.FORM_PLAIN_SKIP for form, _, _, _ in forms), "the plain skip form"
    assert any(not resident for _, _, resident, _ in forms), "a form over a scene that is not resident"
    assert any(not links for _, _, _, links in forms), "a form over a scene with no link table"
    ran = set().union(*(s["resident_walk"] for s in seen))
    want = {"update_device", "rebuild", "pose", "lights", "relink", "a replace that made the scene resident"}
    assert want <= ran, sorted(want - ran)
    print("adaptive list form: ran", sum(s["adaptive"] for s in seen), "times behind an op")
    assert sum(s["adaptive"] for s in seen) > 0


@pytest.mark.parametrize("index", [0, 1])
def test_ops_and_readers_in_stream_order(P, O, index):
    """The same ops and readers enqueued on one side stream with no host wait between an op and the readers behind it, outputs in
    per-step buffers, one synchronize at the end, then the same comparisons.  Calls that synchronise by contract (table reads,
    ptamd_scene_cull_count, margins) are left out; a rebuild, a replace and a change of material tables block by contract and so
    do a rig's creation and destruction, but nothing the test adds waits."""
    import torch
    seq = SEQUENCES[index]
    rs = rays_of(P, O, seq.start)
    with P.Context(0) as ctx:
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            model = S.Model(P, seq.start, seq.mixed)
            dev = Device(P, ctx, model, stream=st)
            t_range = torch.from_numpy(rs.t_range.copy()).cuda()
            rays_np, rays = rs.rays, torch.from_numpy(rs.rays.copy()).cuda()
            held = []
            for step, kind in enumerate(seq.kinds):
                call = model.apply(kind)
                dev.apply(call, model)
                if kind == "lights":
                    rays_np = rs.aimed_at(model.lights)
                    rays = torch.from_numpy(rays_np).cuda()
                hs = model.scene()
                frames = {name: render(P, ctx, (dev.sid, dev.cid), hs.camera_struct(), getattr(P, name), stream=st, size=S.SIZE)
                          for name in kinds_after(step, False, False)}
                walks, _, _ = dev.allows()
                answers = {walk: (ctx.query_rays(dev.sid, rays, t_range, mode="nearest", walk=walk, stream=st),
                                  ctx.query_rays(dev.sid, rays, t_range, mode="any", walk=walk, stream=st)) for walk in walks}
                held.append((f"{seq} step {step} ({kind}), stream order", hs, rays_np, rays, frames, answers))
        torch.cuda.synchronize()
        for what, hs, rays_np, _, frames, answers in held:
            want = S.expected(P, O, hs, rays_np, rs.t_range)
            for name, fr in frames.items():
                assert_same(fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), *want["frame"], f"{what}: {name} vs the oracle")
            for walk, ((hits, uv), occ) in answers.items():
                same(hits, want["hits"], f"{what}: walk {walk} hits")
                same(uv, want["uv"], f"{what}: walk {walk} uv")
                same(occ.view(torch.uint8), want["occluded"], f"{what}: walk {walk} occluded")
        assert ctx.device_error_count() == 0
        dev.close()
