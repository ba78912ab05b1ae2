"""Adaptive sampling that stops and continues on the device (chunky_render_adaptive_ex / _resume / _state / _restore; csrc/adaptive.hip
adaptive_count_kernel) against its specification, bit for bit in image, counts, (m, M2) and the cumulative summary:

  P1  the state after a stop at d passes is chunky_adaptive_host(samples[:d]);
  P2  a run split anywhere — by its own max_spp, by post_render, by a state saved and restored on another target — ends as
      chunky_adaptive_host(samples) does.

The splits are not degenerate (tests/test_adaptive_resume_cpu.py checks the same condition without a device): at every split after
min_spp between 10 % and 90 % of the pixels are still active, so both the list route and the pixels that left are in play."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library loads: torch brings a HIP runtime of its own, and the second runtime of a process finds no device

import golden_scenes as gs
from chunkyclplugin_amd import native
from chunkyclplugin_amd.renderer import RendererInstance
from test_adaptive_cpu import MAX_SPP, SETTINGS, params, samples_of
from test_adaptive_resume_cpu import GPU_SPLITS, GPU_STOPS, same_summary, split_run
from test_gpu_adaptive import SEEDS, bits, close, device_samples, expect_state, make, same

pytestmark = pytest.mark.gpu


def whole(r):
    """(image, counts, noise) of the target."""
    return r.read().reshape(r.height, r.width, 3).copy(), r.adaptive_counts(), r.adaptive_noise()


def equals_host(r, want, what):
    image, counts, noise = whole(r)
    wc, wimg, wst = want
    if not np.array_equal(counts, wc):
        pytest.fail(f"{what}: counts differ at {int((counts != wc).sum())} of {wc.size} pixels; device {np.unique(counts).tolist()}, host {np.unique(wc).tolist()}")
    same(noise, wst, what + " (m, M2)")
    same(image, wimg, what + " image")


def single_run_summary(s, p):
    return split_run(s, p, [s.shape[0]]).summary


_host = {}


def host(name, setting, n):
    """chunky_adaptive_host on the first n oracle samples of a golden scene: computed once, shared."""
    key = (name, setting, n)
    if key not in _host:
        _host[key] = native.adaptive_host(samples_of(name)[:n], params(*setting))
    return _host[key]


@pytest.mark.parametrize("name,setting,a", [(name, setting, a) for name, setting, splits in GPU_SPLITS for a in splits])
def test_split_runs_equal_the_specification(gpu_instance, port, name, setting, a):
    sc = gs.make(name)
    s = samples_of(name, port)
    p = params(*setting)
    loader, r = make(gpu_instance, sc)
    finished, _ = r.render_adaptive_ex(SEEDS[:a], p)
    assert finished
    wa = host(name, setting, a)
    share = float((wa[0] == a).mean())
    print(f"{name} {setting} A = {a}: {share:.4f} of the pixels still active")
    assert share == 1.0 if a == setting[0] else 0.1 <= share <= 0.9, share
    run = r.adaptive_state()
    native.adaptive_state_check(run)
    assert run.state.passes == a and run.state.active == int((wa[0] == a).sum())
    assert np.array_equal(run.active == 1, wa[0] == a)  # the check at A itself has not run: who would leave there is still active
    equals_host(r, wa, f"{name} P1 at {a}")
    finished, summary = r.resume_adaptive(SEEDS, p)
    assert finished
    equals_host(r, host(name, setting, MAX_SPP), f"{name} {a} -> {MAX_SPP}")
    same_summary(summary, single_run_summary(s, p), f"{name} {a}")
    end = r.adaptive_state()
    native.adaptive_state_check(end)
    assert end.summary == summary
    info = r.kernel_info()
    assert info["pool"] >= 0 and info["bvh"] == (name == "entities"), info
    close(r, loader)


class Stop:
    """post_render that asks to stop at its k-th poll."""

    def __init__(self, k):
        self.k, self.polls = k, 0

    def __call__(self):
        self.polls += 1
        return self.polls == self.k


# polls of a run of rounds that fit one launch each: before the launch of round 1 (0 passes), after the check at 8, before the
# launch of round 2, after the check at 12, ...
@pytest.mark.parametrize("k,passes", [(1, 0), (2, 8), (3, 8), (6, 16), (11, 24)])
def test_post_render_stops_the_run_and_resume_finishes_it(gpu_instance, port, k, passes):
    name, setting = "outdoor", SETTINGS[0]
    sc = gs.make(name)
    s = samples_of(name, port)
    p = params(*setting)
    loader, r = make(gpu_instance, sc)
    stop, rounds = Stop(k), []
    finished, summary = r.render_adaptive_ex(SEEDS, p, post_render=stop, round_done=lambda n, active: rounds.append((n, active)))
    assert not finished and stop.polls == k
    run = r.adaptive_state()
    native.adaptive_state_check(run)
    assert run.state.passes == passes and summary["passes"] == passes and run.summary == summary
    if passes >= setting[0]:
        equals_host(r, host(name, setting, passes), f"P1 after a stop at poll {k}")
        if passes > setting[0]:  # a split like any other: not degenerate
            share = float((host(name, setting, passes)[0] == passes).mean())
            print(f"{name} {setting} stop at {passes}: {share:.4f} of the pixels still active")
            assert (name, setting) == GPU_STOPS[:2] and passes in GPU_STOPS[2] and 0.1 <= share <= 0.9, share
        assert run.state.last_check == passes  # stopped after the check
        assert [n for n, _ in rounds] == list(range(setting[0], passes + 1, setting[1])) and [a for _, a in rounds] == summary["active"]
    else:
        assert (run.count == 0).all() and not r.read().any() and rounds == []
    finished, summary = r.resume_adaptive(SEEDS, p, round_done=lambda n, active: rounds.append((n, active)))
    assert finished
    equals_host(r, host(name, setting, MAX_SPP), f"P2 after a stop at poll {k}")
    one = single_run_summary(s, p)
    same_summary(summary, one, f"stop at poll {k}")
    assert [n for n, _ in rounds] == list(range(setting[0], summary["passes"], setting[1])) + [summary["passes"]]
    assert [a for _, a in rounds][:len(one["active"])] == one["active"]
    close(r, loader)


def test_a_stop_inside_a_round(gpu_instance):
    """A first round longer than one launch, stopped at the poll before its second launch: the state is off every check point, below
    min_spp, and all of it continues.  The per-pass samples are one-pass device renders (tests/test_gpu_adaptive.py device_samples).
    Threshold 0.03, chosen on the CPU oracle: after more than a thousand passes nothing is left at 0.2; at 0.03 the check at min_spp
    lets 46 % of the pixels go."""
    sc = gs.make("outdoor")
    loader, r = make(gpu_instance, sc)
    l2, plain = make(gpu_instance, sc)
    mn = r.kernel_info()["passes_per_launch"] + 44
    n = mn + 8
    seeds = native.java_random_ints(n)
    p = params(mn, 4, 0.03)
    s = device_samples(plain, seeds)
    stop = Stop(2)
    finished, summary = r.render_adaptive_ex(seeds, p, post_render=stop)
    assert not finished and stop.polls == 2
    run = r.adaptive_state()
    native.adaptive_state_check(run)
    d = run.state.passes
    assert 0 < d < mn and (run.count == d).all() and run.active.all() and run.state.last_check == 0 and summary["checks"] == 0
    plain.reset()
    plain.render_passes(seeds[:d])
    same(run.mean, plain.read().reshape(run.mean.shape), f"the image after the {d} passes of the first launch")
    finished, summary = r.resume_adaptive(seeds, p)
    assert finished
    want = native.adaptive_host(s, p)
    equals_host(r, want, "P2 after a stop inside the first round")
    same_summary(summary, single_run_summary(s, p), "stop inside a round")
    assert summary["checks"] == 2 and 0.1 <= float((want[0] == n).mean()) <= 0.9, summary  # the list route rendered the last passes
    close(r, loader, plain, l2)


@pytest.mark.parametrize("own_buffer", [False, True])
def test_a_saved_state_continues_on_another_target(gpu_instance, port, own_buffer):
    name, setting, a = "outdoor", SETTINGS[0], 13
    sc = gs.make(name)
    s = samples_of(name, port)
    p = params(*setting)
    l1, r1 = make(gpu_instance, sc)
    assert r1.render_adaptive_ex(SEEDS[:a], p)[0]
    saved = r1.adaptive_state()
    close(r1, l1)
    assert 0.1 <= saved.state.active / saved.count.size <= 0.9
    l2, r2 = make(gpu_instance, sc)
    if own_buffer:
        fb = torch.full((3 * sc.width * sc.height,), 3.5, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r2.set_device_buffer(fb.data_ptr())
    r2.restore_adaptive(saved)
    again = r2.adaptive_state()  # state -> restore -> state: the same bytes
    assert again.header_bytes() == saved.header_bytes()
    for x, y in ((again.mean, saved.mean), (again.count, saved.count), (again.stat, saved.stat), (again.active, saved.active)):
        assert x.tobytes() == y.tobytes()
    finished, summary = r2.resume_adaptive(SEEDS, p)
    assert finished
    equals_host(r2, host(name, setting, MAX_SPP), "restored on another target")
    same_summary(summary, single_run_summary(s, p), "restored")
    if own_buffer:
        torch.cuda.synchronize()
        assert np.array_equal(bits(fb.cpu().numpy()), bits(host(name, setting, MAX_SPP)[1].reshape(-1)))
        r2.set_device_buffer(None)
    close(r2, l2)


RAGGED = (530, 517)  # 34 x 33 = 1122 tiles of 16 x 16, the right and bottom ones partial: the scan's second trip of 1024 runs


def ragged_state(sc, mean, share=0.37):
    """A hand-made state after 4 passes and the check there: a seeded random `share` of the pixels active."""
    w, h = sc.width, sc.height
    st = native.AdaptiveState()
    st.size = C.sizeof(native.AdaptiveState)
    st.width, st.height, st.passes, st.last_check = w, h, 4, 4
    st.params = params(4, 1 << 20, SETTINGS[0][2])
    active = (np.random.default_rng(37).random((h, w)) < share).astype(np.uint8)
    st.active = int(active.sum())
    st.summary.rounds, st.summary.checks, st.summary.passes, st.summary.samples = 1, 1, 4, 4 * w * h
    st.summary.active[0] = st.active
    return native.AdaptiveRun(st, mean, np.full((h, w), 4, np.int32), np.zeros((h, w, 2), np.float32), active)


_ragged = {}


def ragged_reference(gpu_instance):
    """The uniform images after 4 and after 7 passes of the ragged view: rendered once, shared, left unchanged."""
    if not _ragged:
        sc = gs.timed_view("outdoor").with_view(*RAGGED)
        seeds = native.java_random_ints(7)
        loader, r = make(gpu_instance, sc)
        r.render_passes(seeds[:4])
        four = r.read().reshape(sc.height, sc.width, 3).copy()
        r.reset()
        r.render_passes(seeds)
        seven = r.read().reshape(sc.height, sc.width, 3).copy()
        close(r, loader)
        for a in (four, seven):
            a.setflags(write=False)
        _ragged.update(sc=sc, seeds=seeds, four=four, seven=seven)
    return _ragged


def restore_and_resume(gpu_instance, ref):
    sc, seeds = ref["sc"], ref["seeds"]
    run = ragged_state(sc, ref["four"])
    loader, r = make(gpu_instance, sc)
    r.restore_adaptive(run)
    finished, summary = r.resume_adaptive(seeds, run.state.params)
    assert finished and summary["passes"] == 7 and summary["checks"] == 1 and summary["samples"] == 4 * run.count.size + 3 * run.state.active
    out = whole(r)
    assert r.kernel_info()["pool"] >= 0
    close(r, loader)
    return run, out


def test_the_list_rebuilt_from_a_restored_map(gpu_instance):
    """The rebuild on its own — a map no check of this run made, ragged edges, more than 1024 tiles: the pixels of the map, and only
    they, get passes 4 .. 6."""
    ref = ragged_reference(gpu_instance)
    run, (image, counts, noise) = restore_and_resume(gpu_instance, ref)
    on = run.active == 1
    assert 0.3 < on.mean() < 0.45 and (ref["sc"].width % 16 and ref["sc"].height % 16)
    assert np.array_equal(counts, np.where(on, 7, 4))
    same(image[on][None], ref["seven"][on][None], "active pixels against 7 uniform passes")
    same(image[~on][None], ref["four"][~on][None], "inactive pixels keep the restored bits")
    assert not noise[~on].any() and np.isfinite(noise[on]).all()


def test_restore_and_resume_twice_give_identical_bytes(gpu_instance):
    ref = ragged_reference(gpu_instance)
    _, a = restore_and_resume(gpu_instance, ref)
    _, b = restore_and_resume(gpu_instance, ref)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def expect_invalid(fn):
    with pytest.raises(native.ChunkyHipError) as e:
        fn()
    assert e.value.code == native.E_INVALID, e.value


def test_what_ends_a_state(gpu_instance):
    sc = gs.make("outdoor")
    p = params(*SETTINGS[0])
    loader, r = make(gpu_instance, sc)
    expect_state(lambda: r.resume_adaptive(SEEDS, p))  # no state yet
    expect_state(r.adaptive_state)
    buffer = np.zeros(sc.width * sc.height * 3, np.float64)
    enders = {
        "render_passes": lambda: r.render_passes(SEEDS[:1]),
        "render_run": lambda: r.render(buffer, 0, 1),
        "render_run_ex": lambda: r.render_ex(buffer, 0, 1),
        "render_reset": r.reset,
        "selftest_render_list": lambda: r.render_list(np.arange(5, dtype=np.int32), SEEDS[:1]),
        "set_device_buffer": lambda: r.set_device_buffer(None),
        "set_camera": lambda: r.set_camera(sc.projector_type, sc.camera),
        "set_option": lambda: r.set_option(native.OPT_KERNEL, 0),
        "set_shard": lambda: r.set_shard(0, 1, 256),
    }
    for what, end in enders.items():
        assert r.render_adaptive_ex(SEEDS[:12], p)[0]
        counts, noise = r.adaptive_counts(), r.adaptive_noise()
        r.adaptive_state()
        r.render_aov(SEEDS[:2])  # the AOV and denoise calls do not end it
        r.denoise()
        assert r.adaptive_state().state.passes == 12
        end()
        with pytest.raises(native.ChunkyHipError) as e:
            r.resume_adaptive(SEEDS, p)
        assert e.value.code == native.E_STATE, (what, e.value)
        with pytest.raises(native.ChunkyHipError) as e:
            r.adaptive_state()
        assert e.value.code == native.E_STATE, (what, e.value)
        if what != "selftest_render_list":  # (that call overwrites the statistic, as before)
            assert np.array_equal(r.adaptive_counts(), counts) and np.array_equal(bits(r.adaptive_noise()), bits(noise)), what  # the maps stay readable, as before
    close(r, loader)


def test_argument_and_state_errors(gpu_instance, port):
    name, setting = "outdoor", SETTINGS[0]
    sc = gs.make(name)
    p = params(*setting)
    loader, r = make(gpu_instance, sc)
    assert r.render_adaptive_ex(SEEDS[:13], p)[0]
    before = r.adaptive_state()
    for other in (params(8, 4, 0.25), params(8, 4, 0.2, floor=0.02), params(9, 4, 0.2), params(8, 5, 0.2)):
        expect_state(lambda: r.resume_adaptive(SEEDS, other))  # other parameters than the state's
    expect_invalid(lambda: r.resume_adaptive(SEEDS[:12], p))  # max_spp < passes
    finished, summary = r.resume_adaptive(SEEDS[:13], p)  # max_spp == passes: nothing happens
    assert finished and summary == before.summary
    same_state = r.adaptive_state()
    assert same_state.header_bytes() == before.header_bytes() and same_state.mean.tobytes() == before.mean.tobytes()
    # restore: a state of another size, and an invalid one, leave the target as it was
    small = split_run(samples_of(name, port)[:, :32, :32], p, [13])
    expect_invalid(lambda: r.restore_adaptive(small))
    bad = before.copy()
    bad.state.active += 1
    expect_invalid(lambda: r.restore_adaptive(bad))
    bad = before.copy()
    bad.count[0, 0] += 1
    expect_invalid(lambda: r.restore_adaptive(bad))
    still = r.adaptive_state()
    assert still.header_bytes() == before.header_bytes()
    for x, y in ((still.mean, before.mean), (still.count, before.count), (still.stat, before.stat), (still.active, before.active)):
        assert x.tobytes() == y.tobytes()
    assert r.resume_adaptive(SEEDS, p)[0]
    equals_host(r, host(name, setting, MAX_SPP), "after the refused calls")
    # a sharded target
    r.restore_adaptive(before)
    r.set_shard(0, 2, 0)
    expect_state(lambda: r.resume_adaptive(SEEDS, p))
    expect_state(r.adaptive_state)
    expect_state(lambda: r.restore_adaptive(before))
    r.set_shard(0, 1, 256)
    expect_state(lambda: r.resume_adaptive(SEEDS, p))  # the state stays ended
    cb = native.AdaptiveCallbacks()  # a callbacks struct that cuts a member in half
    cb.struct_size = C.sizeof(C.c_size_t) + 4
    s32 = np.ascontiguousarray(SEEDS, np.int32)
    assert native.lib().chunky_render_adaptive_ex(r._h, native.ptr(s32), s32.size, C.byref(p), C.byref(cb), None) == native.E_INVALID
    close(r, loader)
    g = RendererInstance.group([0, 0])  # a group's target
    loader, r = make(g, sc)
    expect_state(lambda: r.render_adaptive_ex(SEEDS, p))
    expect_state(lambda: r.resume_adaptive(SEEDS, p))
    expect_state(r.adaptive_state)
    expect_state(lambda: r.restore_adaptive(before))
    close(r, loader)
    g.close()
