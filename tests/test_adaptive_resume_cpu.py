"""Adaptive sampling that stops and continues, without a device (chunky_adaptive_host_begin / _resume / chunky_adaptive_state_check;
csrc/adaptive_spec.h ad_step) against the single run chunky_adaptive_host on the oracle's per-pass samples, bit for bit:

  P1  stop = shorter run: the state after d >= min_spp passes is chunky_adaptive_host(samples[:d]);
  P2  resume = fresh: the start state continued over any split of the passes is chunky_adaptive_host(samples), and the summary's
      checks, active[], samples and passes are the single run's.

Every two-way split of the 40 passes and three three-way splits, on all ten golden scenes under the setting that carries each
(tests/test_adaptive_cpu.py CARRIES).  The sweep is exhaustive so that it holds the degenerate splits too (before min_spp, on and off
the grid, after every pixel has left); the splits the device tests use (tests/test_gpu_adaptive_resume.py) are checked here for NOT
being degenerate: between 10 % and 90 % of the pixels are still active at the split."""
import ctypes as C

import numpy as np
import pytest

import adaptive_spec as sp
import golden_scenes as gs
from chunkyclplugin_amd import native
from test_adaptive_cpu import CARRIES, FLOOR, MAX_SPP, SETTINGS, bits, params, samples_of

# (scene, setting, splits): what tests/test_gpu_adaptive_resume.py runs; A = min_spp is the all-active case and exempt from the condition
GPU_SPLITS = [("outdoor", SETTINGS[0], (8, 12, 13, 20, 39)), ("entities", SETTINGS[0], (8, 12, 13, 20, 39)),
              ("pregen", SETTINGS[0], (8, 12, 13, 20, 39)), ("inside", SETTINGS[1], (17, 28, 29))]
GPU_STOPS = ("outdoor", SETTINGS[0], (16, 24))  # ... and where its post_render stops land after min_spp
THREE_WAY = [(8, 13, 40), (12, 20, 40), (5, 8, 40)]


def setting_of(name):
    return SETTINGS[CARRIES[name]]


def same_arrays(run, want, what):
    wc, wimg, wst = want
    assert np.array_equal(run.count, wc), f"{what}: counts differ at {int((run.count != wc).sum())} pixels"
    assert np.array_equal(bits(run.mean), bits(wimg)), f"{what}: image"
    assert np.array_equal(bits(run.stat), bits(wst)), f"{what}: (m, M2)"


def same_summary(got, single, what):
    for key in ("checks", "active", "samples", "passes"):
        assert got[key] == single[key], (what, key, got, single)


def split_run(s, p, cuts, visit=None):
    """begin, then resume over the passes [0, cuts[0]), [cuts[0], cuts[1]), ...; visit(run, d) sees the state after each cut."""
    run = native.adaptive_host_begin(s.shape[2], s.shape[1], p)
    native.adaptive_state_check(run)
    d0 = 0
    for d in cuts:
        native.adaptive_host_resume(run, s[d0:d])
        native.adaptive_state_check(run)
        if visit:
            visit(run, d)
        d0 = d
    return run


def active_share(s, p, a):
    """The share of the pixels whose count in chunky_adaptive_host(samples[:a]) equals a: those a run split at a still renders."""
    return float((native.adaptive_host(s[:a], p)[0] == a).mean())


@pytest.mark.parametrize("name", gs.NAMES)
def test_every_split_equals_the_single_run(port, name):
    s = samples_of(name, port)
    mn, ci, thr = setting_of(name)
    p = params(mn, ci, thr)
    full = native.adaptive_host(s, p)
    trace = []
    sp.adaptive(s, thr, FLOOR, mn, ci, trace)
    single = split_run(s, p, [MAX_SPP])
    same_arrays(single, full, f"{name}: one resume over all passes")
    one = single.summary
    assert one["samples"] == int(full[0].sum()) and one["passes"] == int(full[0].max()) and one["active"] == trace and one["checks"] == len(trace), one
    shorter = {d: native.adaptive_host(s[:d], p) for d in range(mn, MAX_SPP + 1)}

    def p1(run, d):
        st = run.state
        if st.active == 0:
            assert st.passes <= d and st.passes == int(run.count.max())
        else:
            assert st.passes == d
        if d < mn:  # nothing is checked before min_spp: every count is the pass count
            assert (run.count == d).all() and st.active == run.count.size and st.last_check == 0
            assert np.array_equal(bits(run.mean), bits(sp.running_mean(s, d)))
        else:
            same_arrays(run, shorter[d], f"{name}: P1 at {d}")

    for d in range(1, MAX_SPP):
        run = split_run(s, p, [d, MAX_SPP], p1)
        same_arrays(run, full, f"{name}: split at {d}")
        same_summary(run.summary, one, f"{name}: split at {d}")
    for cuts in THREE_WAY:
        run = split_run(s, p, cuts, p1)
        same_arrays(run, full, f"{name}: split {cuts}")
        same_summary(run.summary, one, f"{name}: split {cuts}")


def test_the_device_tests_splits_are_not_degenerate(port):
    for name, setting, splits in GPU_SPLITS + [GPU_STOPS]:
        s = samples_of(name, port)
        for a in splits:
            share = active_share(s, params(*setting), a)
            if a == setting[0]:
                assert share == 1.0, (name, a, share)  # A = min_spp: the all-active case
            else:
                assert 0.1 <= share <= 0.9, (name, setting, a, share)


def test_a_state_whose_pixels_have_all_left_resumes_to_itself():
    s = np.full((20, 6, 7, 3), 0.25, np.float32)  # a constant stream: every pixel leaves at min_spp
    p = params(5, 4, 0.1)
    run = split_run(s, p, [9])
    assert run.state.active == 0 and run.state.passes == 5 and run.state.last_check == 5 and (run.count == 5).all() and not run.active.any()
    before = run.copy()
    native.adaptive_host_resume(run, s[9:])
    assert run.header_bytes() == before.header_bytes()
    for a, b in ((run.mean, before.mean), (run.count, before.count), (run.stat, before.stat), (run.active, before.active)):
        assert a.tobytes() == b.tobytes()
    same_arrays(run, native.adaptive_host(s, p), "constant stream")
    native.adaptive_host_resume(run, s[:0])  # and no pass at all changes nothing either
    assert run.header_bytes() == before.header_bytes()


def invalid(run):
    with pytest.raises(native.ChunkyHipError) as e:
        native.adaptive_state_check(run)
    assert e.value.code == native.E_INVALID, e.value
    return str(e.value)


def test_state_check_rejects_each_broken_rule(port):
    s = samples_of("outdoor", port)
    p = params(*SETTINGS[0])  # grid 8, 12, 16, ...
    good = split_run(s, p, [13])  # off the grid: last_check 12
    st = good.state
    assert st.passes == 13 and st.last_check == 12 and 0 < st.active < good.count.size
    on = np.argwhere(good.active.reshape(-1) == 1)[0, 0]
    off = np.argwhere(good.active.reshape(-1) == 0)[0, 0]

    def broken(change):
        run = good.copy()
        change(run)
        return invalid(run)

    def set_count(i, v):  # (summary.samples follows: one rule broken at a time)
        def change(run):
            run.state.summary.samples += v - int(run.count.reshape(-1)[i])
            run.count.reshape(-1)[i] = v
        return change

    assert "active with count" in broken(set_count(on, 12))  # an active pixel with count != passes
    assert "inactive with count" in broken(set_count(off, 10))  # an inactive count off the grid
    assert "inactive with count" in broken(set_count(off, 16))  # ... on the grid but after the last check
    assert "inactive with count" in broken(set_count(off, 0))  # ... 0 is no check point

    def last_check(v):
        return lambda run: setattr(run.state, "last_check", v)

    for v in (8, 13, 0, 16, -1):  # after 13 passes only 12 is legal
        assert "last_check" in broken(last_check(v)), v

    def map_value(run):
        run.active.reshape(-1)[off] = 2

    assert "not 0 or 1" in broken(map_value)
    assert "state.active" in broken(lambda run: setattr(run.state, "active", run.state.active + 1))
    assert "summary.samples" in broken(lambda run: setattr(run.state.summary, "samples", run.state.summary.samples - 1))
    assert "summary.passes" in broken(lambda run: setattr(run.state.summary, "passes", 12))
    assert "state.size" in broken(lambda run: setattr(run.state, "size", native.AdaptiveState.summary.offset))
    assert "passes" in broken(lambda run: setattr(run.state, "passes", -1))
    assert "bad size" in broken(lambda run: setattr(run.state, "width", 0))
    for member, v in (("threshold", -0.1), ("threshold", float("nan")), ("floor", 0.0), ("min_spp", 1), ("check_interval", 0), ("flags", 1)):
        assert "adaptive_state_check" in broken(lambda run: setattr(run.state.params, member, v)), member
    assert "params.size" in broken(lambda run: setattr(run.state.params, "size", native.AdaptiveParams.flags.offset))
    # on a grid point both the point (its check has run) and the one before it (it has not) are legal, nothing else
    at = split_run(s, p, [12])
    assert at.state.last_check == 8
    for v, ok in ((8, True), (12, True), (0, False), (4, False), (16, False)):
        run = at.copy()
        run.state.last_check = v
        if ok:
            native.adaptive_state_check(run)
        else:
            assert "last_check" in invalid(run)
    first = split_run(s, p, [8])  # the first grid point: 0 (none yet) or 8
    assert first.state.last_check == 0
    first.state.last_check = 8
    native.adaptive_state_check(first)
    L = native.lib()
    assert L.chunky_adaptive_state_check(None, native.ptr(good.count), native.ptr(good.active)) == native.E_INVALID
    assert L.chunky_adaptive_state_check(C.byref(good.state), None, native.ptr(good.active)) == native.E_INVALID
    # resume validates first, and begin takes the parameter rules without the pass count
    bad = good.copy()
    bad.state.active += 1
    with pytest.raises(native.ChunkyHipError) as e:
        native.adaptive_host_resume(bad, s[13:])
    assert e.value.code == native.E_INVALID
    with pytest.raises(native.ChunkyHipError) as e:
        native.adaptive_host_begin(4, 4, params(1, 4, 0.1))
    assert e.value.code == native.E_INVALID


def test_the_step_function_on_hand_written_cases():
    """ad_step is not exported: its decisions are read off one-step resumes of a 1 x 1 state (summary.checks and passes)."""
    def steps(passes, last_check, mn, ci, max_spp):
        # a noisy pixel that never converges at threshold 0: every step the loop takes shows in rounds / checks
        rng = np.random.default_rng(5)
        s = np.abs(rng.normal(0.5, 0.3, size=(max_spp, 1, 1, 3))).astype(np.float32)
        p = params(mn, ci, 0.0)
        run = native.adaptive_host_begin(1, 1, p)
        native.adaptive_host_resume(run, s[:passes])
        if last_check is not None:
            run.state.last_check = last_check
            native.adaptive_state_check(run)
        base = run.summary
        native.adaptive_host_resume(run, s[passes:max_spp])
        after = run.summary
        return after["rounds"] - base["rounds"], after["checks"] - base["checks"], run.state.passes, run.state.last_check

    # on the grid, its check not run (the earlier run ended there): the check first, then one round to 16 and its check
    assert steps(12, 8, 8, 4, 20) == (2, 2, 20, 16)  # checks at 12 (first) and 16, rounds 12-16 and 16-20, no check at 20 = max_spp
    assert steps(12, 8, 8, 4, 16) == (1, 1, 16, 12)  # the check at 12, one round, no check at max_spp
    # on the grid, checked: straight to the round
    assert steps(12, 12, 8, 4, 16) == (1, 0, 16, 12)
    assert steps(12, 12, 8, 4, 17) == (2, 1, 17, 16)
    # off the grid: a short round to the next grid point first
    assert steps(13, None, 8, 4, 16) == (1, 0, 16, 12)
    assert steps(13, None, 8, 4, 21) == (3, 2, 21, 20)  # 13-16 check, 16-20 check, 20-21
    assert steps(13, None, 8, 4, 14) == (1, 0, 14, 12)
    # below min_spp: to min_spp (or to max_spp when that comes first), nothing checked on the way
    assert steps(3, None, 8, 4, 9) == (2, 1, 9, 8)
    assert steps(3, None, 8, 4, 8) == (1, 0, 8, 0)
    assert steps(3, None, 8, 4, 5) == (1, 0, 5, 0)
    assert steps(0, None, 8, 4, 16) == (3, 2, 16, 12)  # the single run: 8, then 4 at a time
    # one pass left
    assert steps(15, None, 8, 4, 16) == (1, 0, 16, 12)
    assert steps(16, 12, 8, 4, 17) == (1, 1, 17, 16)
    assert steps(16, 16, 8, 4, 17) == (1, 0, 17, 16)
    # a very long interval cannot overflow the step
    assert steps(5, None, 4, 2 ** 31 - 1, 9) == (1, 0, 9, 4)
