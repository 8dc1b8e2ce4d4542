"""Launch lanes (ptamd_host.h: ptamd_context::lane): megakernels of launches with machine_share > 1 and of a
host running ahead on one stream go to streams the context owns, each with a hardware queue of its own; resolve passes stay
on the caller's stream.  Every case holds frames rendered that way to the same frames rendered on one stream, one frame per
launch, with the host waiting for each: accumulators and surfaces bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, B = 480, 270, 4


def assert_same(acc, rgba, ref_acc, ref_rgba, what=""):
    bad = (acc.view(np.uint32) != ref_acc.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} accumulator pixels differ (first {np.argwhere(bad)[:3].tolist()})"
    np.testing.assert_array_equal(rgba, ref_rgba, err_msg=what)


@pytest.fixture
def scene(P, indoor):
    """A context of its own (lanes 3 and 4 are created per context) with the indoor scene uploaded."""
    ctx = P.Context(0)
    ids = (ctx.upload_scene(indoor), ctx.upload_cubemap(P.cubemap_for_scene(indoor)))
    yield ctx, ids, indoor.camera_struct()
    ctx.close()


def reference(P, ctx, ids, cam, plan):
    """plan: (first frame, frames, reset) per step.  One frame per launch on the current stream, the host waiting for each."""
    import torch
    fr = P.FrameRenderer(ctx, *ids, cam, W, H)
    for first, n, reset in plan:
        for k in range(first, first + n):
            l = ctx.make_launch(fr.surface, fr.accum, *ids, cam, W, H, frame_nb=k, bounces=B,
                                reset_accumulation=reset and k == first, no_pipelining=True)
            ctx.raytrace_ex(l)
            torch.cuda.synchronize()
    return fr.accum.cpu().numpy(), fr.surface.cpu().numpy()


def run_in_flight(P, ctx, ids, cam, plans, share):
    """plans[i]: the steps of renderer i on stream i; steps are issued round-robin over the renderers, host never waiting."""
    import torch
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in plans]
    frs = [P.FrameRenderer(ctx, *ids, cam, W, H, machine_share=share) for _ in plans]
    torch.cuda.synchronize()
    for j in range(max(len(p) for p in plans)):
        for fr, st, plan in zip(frs, streams, plans):
            if j < len(plan):
                first, n, reset = plan[j]
                with torch.cuda.stream(st):
                    fr.render(spp=n, bounces=B, first_frame=first, batched=True, stream=st, reset=reset)
    torch.cuda.synchronize()
    return [(fr.accum.cpu().numpy(), fr.surface.cpu().numpy()) for fr in frs]


def test_two_streams_half_machine(P, scene):
    """Two caller streams, machine_share = 2: six batched 4-frame steps alternating between them, some starting a new
    accumulation and some adding to the last one."""
    ctx, ids, cam = scene
    plans = [[(1, 4, True), (5, 4, False), (9, 4, True)],
             [(21, 4, True), (25, 4, False), (29, 4, False)]]
    got = run_in_flight(P, ctx, ids, cam, plans, 2)
    for i, plan in enumerate(plans):
        assert_same(*got[i], *reference(P, ctx, ids, cam, plan), f"stream {i} of 2, machine_share 2")


def test_four_streams_quarter_machine(P, scene):
    """Four caller streams, machine_share = 4: the launch that brings lanes 3 and 4 into being and those after it."""
    ctx, ids, cam = scene
    plans = [[(1 + 40 * i, 4, True), (5 + 40 * i, 4, i % 2 == 0), (9 + 40 * i, 4, False)] for i in range(4)]
    got = run_in_flight(P, ctx, ids, cam, plans, 4)
    for i, plan in enumerate(plans):
        assert_same(*got[i], *reference(P, ctx, ids, cam, plan), f"stream {i} of 4, machine_share 4")


def test_long_batches_on_two_streams(P, scene):
    """frame_count = 13 (four parts of at most four frames inside the library) on two caller streams, machine_share = 2,
    pipelining allowed: every part after a stream's first takes a lane."""
    ctx, ids, cam = scene
    plans = [[(1, 13, True), (14, 13, False)],
             [(101, 13, True), (114, 13, True)]]
    got = run_in_flight(P, ctx, ids, cam, plans, 2)
    for i, plan in enumerate(plans):
        assert_same(*got[i], *reference(P, ctx, ids, cam, plan), f"stream {i}, frame_count 13")


def test_captured_half_machine_launch_stays_on_the_callers_stream(P, scene):
    """A machine_share = 2 launch captured into a graph runs on the capturing stream (a lane is never captured) and every
    replay produces the eager launch's accumulator and surface."""
    import torch
    ctx, ids, cam = scene
    want = reference(P, ctx, ids, cam, [(1, 4, True)])
    fr = P.FrameRenderer(ctx, *ids, cam, W, H, machine_share=2)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        # warm-up: the stream's first launch sizes its own slab, the second one runs its megakernel on a lane
        for _ in range(2):
            fr.render(spp=4, bounces=B, batched=True, reset=True, stream=side)
    torch.cuda.synchronize()
    assert_same(fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), *want, "eager machine_share 2")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fr.render(spp=4, bounces=B, batched=True, reset=True, stream=torch.cuda.current_stream())
    for rep in range(3):
        fr.accum.fill_(7.0)
        fr.surface.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert_same(fr.accum.cpu().numpy(), fr.surface.cpu().numpy(), *want, f"graph replay {rep}")
    del g
    torch.cuda.synchronize()
    ctx.release_captured(side)


def test_contexts_come_and_go_with_launches_in_flight(P, indoor):
    """Twenty contexts, each destroyed with launches still in flight on two streams: no error, and the device's free memory
    returns to within 64 MB of where it started (lanes, slabs and events go with their context)."""
    import torch
    dev = torch.device("cuda", 0)
    cube = P.cubemap_for_scene(indoor)
    cam = indoor.camera_struct()
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    bufs = [(torch.zeros((H, W, 4), dtype=torch.uint8, device=dev), torch.zeros((H, W, 3), dtype=torch.float32, device=dev))
            for _ in streams]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info(dev)
    for rep in range(20):
        ctx = P.Context(0)
        ids = (ctx.upload_scene(indoor), ctx.upload_cubemap(cube))
        for step in range(3):
            for (surface, accum), st in zip(bufs, streams):
                l = ctx.make_launch(surface, accum, *ids, cam, W, H, frame_nb=1 + 4 * step, bounces=B, stream=st,
                                    frame_count=4, machine_share=2, reset_accumulation=True)
                ctx.raytrace_ex(l)
        ctx.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free1, _ = torch.cuda.mem_get_info(dev)
    assert free1 >= free0 - (64 << 20), f"free device memory {free0 >> 20} MB -> {free1 >> 20} MB after 20 contexts"
