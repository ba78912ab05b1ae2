"""The convergence kernels of adaptive sampling (csrc/adaptive.hip) at their edges: images narrower or lower than one 16 x 16 tile,
ragged in one pixel, exactly 1023 / 1024 / 1025 / 2049 tiles (adaptive_scan_kernel takes 1024 tile counts at a time and carries a
running total across), the parameters at the ends of their ranges, and a second run on a target whose list still holds a longer
first run.  Reference: chunky_adaptive_host on the oracle's per-pass samples (check_against_samples of tests/test_gpu_adaptive.py),
bit for bit, and the active pixels after every check.  The settings, and the condition that a case really runs the list route
(three distinct counts, 10 - 90 % of the pixels leave early, some stay to the end), come from tests/test_list_route_cpu.py, which
asserts the condition on the host; it is asserted on the device run here."""
import numpy as np
import pytest

import golden_scenes as gs
from chunkyclplugin_amd import native
from test_adaptive_cpu import MAX_SPP, params, samples_of
from test_gpu_adaptive import bits, check_against_samples, close, make
from test_list_route_cpu import (ALL_LEAVE, NONE_LEAVES, PARAM_EDGES, PREGEN_VIEW, SCAN_SETTING, SCAN_SPP, SCAN_WIDTHS, SMALL_SETTING,
                                 SMALL_SIZES, TOO_SMALL, TWO_RUNS, check_points, edge_samples, host_active, non_degenerate, pregen_scene,
                                 scan_scene, small_scene)

pytestmark = pytest.mark.gpu
SEEDS = native.java_random_ints(MAX_SPP)


def run(gpu_instance, sc, s, setting, what, condition=True, kernel=None):
    """One adaptive run of sc against the host on the samples s; the active pixels after every check are the host's."""
    max_spp = s.shape[0]
    loader, r = make(gpu_instance, sc)
    counts, summary = check_against_samples(r, s, SEEDS[:max_spp], params(*setting), what)
    info = r.kernel_info()
    close(r, loader)
    want = host_active(native.adaptive_host(s, params(*setting))[0], setting, max_spp)
    assert summary["checks"] == len(want) and summary["active"] == want, (what, summary, want)
    if condition:
        assert non_degenerate(counts, max_spp, summary["active"][-1]), (what, np.unique(counts).tolist(), summary)
    if kernel:
        assert (info["tree"], info["pool"], info["bvh"]) == kernel, info
    return counts, summary


@pytest.mark.parametrize("size", SMALL_SIZES, ids=[f"{w}x{h}" for w, h in SMALL_SIZES])
@pytest.mark.parametrize("name", sorted(SMALL_SETTING))
def test_small_and_ragged_views(gpu_instance, port, name, size):
    w, h = size
    sc = small_scene(name, w, h)
    s = edge_samples((name, w, h), sc, MAX_SPP, port)
    run(gpu_instance, sc, s, SMALL_SETTING[name], f"{name} {w} x {h}", condition=size not in TOO_SMALL,
        kernel=(16, 64, False) if name == "outdoor" else (-1, 32, True))


def test_pregenerated_rays_on_a_ragged_view(gpu_instance, port):
    sc = pregen_scene()
    run(gpu_instance, sc, edge_samples("pregen17", sc, MAX_SPP, port), PREGEN_VIEW[3], "pregen 17 x 17", kernel=(16, 64, False))


@pytest.mark.parametrize("width", SCAN_WIDTHS)
def test_scan_chunk_edge(gpu_instance, port, width):
    """One tile row of 1023, 1024, 1025 and 2049 tiles (the ABI takes these widths): the offsets of the tiles past the first 1024
    carry the total of the chunks before them."""
    sc = scan_scene(width)
    s = edge_samples(("scan", width), sc, SCAN_SPP, port)
    counts, summary = run(gpu_instance, sc, s, SCAN_SETTING, f"{width} x 1", kernel=(16, 64, False))
    assert summary["checks"] == len(check_points(SCAN_SETTING, SCAN_SPP)) == 4


@pytest.mark.parametrize("what", sorted(PARAM_EDGES))
def test_parameters_at_their_edges(gpu_instance, port, what):
    """check_interval 1, the smallest min_spp the ABI takes (2: it refuses 1), max_spp not a multiple of the interval."""
    max_spp, setting = PARAM_EDGES[what]
    counts, summary = run(gpu_instance, gs.make("outdoor"), samples_of("outdoor", port)[:max_spp], setting, what)
    assert summary["passes"] == max_spp and summary["rounds"] == 1 + len(check_points(setting, max_spp))
    if what == "min-spp-2":
        loader, r = make(gpu_instance, gs.make("outdoor"))
        with pytest.raises(native.ChunkyHipError) as e:
            r.render_adaptive(SEEDS, params(1, 4, 0.2))
        assert e.value.code == native.E_INVALID
        close(r, loader)


def test_every_pixel_leaves_at_the_first_check(gpu_instance, port):
    name, setting = ALL_LEAVE
    counts, summary = run(gpu_instance, gs.make(name), samples_of(name, port), setting, "all leave", condition=False)
    assert (counts == setting[0]).all() and summary["rounds"] == 1 and summary["active"] == [0] and summary["samples"] == counts.size * setting[0]


def test_no_pixel_leaves(gpu_instance, port):
    name, setting = NONE_LEAVES
    counts, summary = run(gpu_instance, gs.make(name), samples_of(name, port), setting, "none leaves", condition=False)
    assert (counts == MAX_SPP).all() and summary["active"] == [counts.size] * len(check_points(setting, MAX_SPP))
    assert summary["samples"] == counts.size * MAX_SPP


def test_a_second_run_does_not_read_the_first_runs_list(gpu_instance, port):
    """Two runs on one target with different parameters, every list of the second shorter than every list of the first: the stale
    tail of the list is not read — counts, statistic and image are a fresh target's (the host's)."""
    sc = gs.make("outdoor")
    s = samples_of("outdoor", port)
    loader, r = make(gpu_instance, sc)
    first, fsum = check_against_samples(r, s, SEEDS, params(*TWO_RUNS[0]), "first run")
    second, ssum = check_against_samples(r, s, SEEDS, params(*TWO_RUNS[1]), "second run on the same target")
    assert ssum["active"] == host_active(second, TWO_RUNS[1], MAX_SPP) and max(ssum["active"]) < min(fsum["active"])
    assert non_degenerate(first, MAX_SPP, fsum["active"][-1]) and non_degenerate(second, MAX_SPP, ssum["active"][-1])
    l2, fresh = make(gpu_instance, sc)
    image, counts, noise, summary = fresh.render_adaptive(SEEDS, params(*TWO_RUNS[1]))
    assert np.array_equal(counts, second) and summary == ssum
    assert np.array_equal(bits(image.reshape(-1)), bits(r.read())) and np.array_equal(bits(noise), bits(r.adaptive_noise()))
    close(r, loader, fresh, l2)
