"""The pixel-list route of render_pool (a temporary ShardView{0, 2, 1, n, list, n}: chunky_selftest_render_list, the rounds of
chunky_render_adaptive after the first check) on every instantiation launch_pool can pick, against the CPU oracle, bit for bit.

One flat matrix, test_list[<scene>-form<tree form>-<kind>-<list>]: each cell renders a hand-made list of pixels into a caller-owned
buffer that holds a marker and asserts that every listed pixel is the oracle's, that every other pixel still holds the marker, and
that kernel_info() names exactly the instantiation the cell is there for (tree form, parked paths, entity-BVH phases, extended
options, sorted block tests) — a cell that ran another kernel fails.  On this route a slot's pixel, its column and row, the
pre-generated ray it reads and the RNG stream it seeds all come from the list entry, so the lists of pre-generated cameras never
hold pixel k in slot k (tests/test_list_route_cpu.py, which also checks the scenes' tree forms and BVH heights on the host).

Block-mapping counterparts: tests/test_gpu_deep_trees.py, test_timed_goldens.py, test_timed_camera_views.py, test_gpu_parity.py."""
import dataclasses
import zlib
from typing import Optional

import numpy as np
import pytest
import torch  # before the library loads: torch brings a HIP runtime of its own, and the second runtime of a process finds no device

import golden_scenes as gs
from chunkyclplugin_amd import native
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader
from oracle.binding import PortExt, PortOptions
from test_list_route_cpu import (BVH_LEAF, NP, PASS_COUNTS, SPLIT_LIST, SPLIT_PASSES, cell_list, pixel_list, scene, shape_lists,
                                 whole_image)

pytestmark = pytest.mark.gpu
SEEDS = native.java_random_ints(SPLIT_PASSES)
MARKER = 7.25
EXT = dict(bsdf=1, nee=1)
EXT_OPTS = {"sun_sampling": native.OPT_SUN_SAMPLING, "emitters": native.OPT_EMITTERS, "bsdf": native.OPT_BSDF, "nee": native.OPT_EMITTER_NEE}
PROJ = {"parallel": native.PROJ_PARALLEL, "fisheye": native.PROJ_FISHEYE, "panoramic": native.PROJ_PANORAMIC,
        "slot": native.PROJ_PANORAMIC_SLOT, "stereographic": native.PROJ_STEREOGRAPHIC}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@dataclasses.dataclass
class Cell:
    id: str
    scene: tuple                    # (golden scene, tree form of its octree[, BVH leaf size]) or ("offset",) / ("any",)
    want: tuple                     # (tree, pool, bvh, ext, sorted) of kernel_info()
    listed: np.ndarray
    passes: int
    variant: int = 0                # OPT_KERNEL
    proj: Optional[str] = None      # a projected camera: proj::render_pool
    ext: Optional[dict] = None      # the extended light-transport options (on materials with specular words)
    opts: Optional[tuple] = None    # (OPT_DRAW_DEPTH, OPT_MAX_DEPTH, OPT_EMITTER_SCALE)


CELLS = []


def add(id_, scene_, want, listed=None, passes=None, **kw):
    """A cell; its list (a permuted subset of 1337 pixels) and its pass count (5 to 9) follow from its id alone."""
    k = zlib.crc32(id_.encode())
    CELLS.append(Cell(id_, scene_, want, cell_list(k % 64) if listed is None else listed, passes or 5 + (k >> 8) % 5, **kw))


def plain(form):
    return (form, 64, False, False, False)


# ---- cameras on the list route, at the one-level forms -----------------------------------------------------------------------------
# (model blocks are common enough in the 8-chunk world that launch_pool sorts its block tests by itself: variant bit 9 keeps the
# form-17 cells on the plain instantiation, the one the timed views run; the sorted one has its own cell below)
for form in (16, 17):
    unsorted = 512 if form == 17 else 0
    for name in ("pregen", "dof", "inside"):
        add(f"{name}-form{form}-plain-permuted-1337", (name, form), plain(form), variant=unsorted)
    for kind in ("parallel", "fisheye", "panoramic", "stereographic"):
        add(f"outdoor-form{form}-{kind}-permuted-1337", ("outdoor", form), plain(form), proj=kind, variant=unsorted)
# ---- tree forms ---------------------------------------------------------------------------------------------------------------------
for form in (18, 19, 0):
    for name in ("outdoor", "pregen"):
        add(f"{name}-form{form}-plain-permuted-1337", (name, form), plain(form))
add("offset-form18-plain-permuted-1337", ("offset",), plain(18))
add("any-form19-plain-permuted-1337", ("any",), plain(19))
add("outdoor-form0-sortbit-permuted-1337", ("outdoor", 0), plain(0), variant=256)  # no sorted instantiation without a wide tree
# ---- kinds --------------------------------------------------------------------------------------------------------------------------
for form in (16, 17, 18, 19):
    add(f"outdoor-form{form}-sorted-permuted-1337", ("outdoor", form), (form, 64, False, False, True), variant=256)
# the 0- and 32-path pools have the generic walk over the wide tree (-1) and the reference layout (0: variant bit 0) only
for bit, pool in ((64, 0), (128, 32)):
    add(f"outdoor-form16-pool{pool}-permuted-1337", ("outdoor", 16), (-1, pool, False, False, False), variant=bit)
    add(f"outdoor-form16-pool{pool}ref-permuted-1337", ("outdoor", 16), (0, pool, False, False, False), variant=1 | bit)
add("pregen-form0-pool0-permuted-1337", ("pregen", 0), (0, 0, False, False, False), variant=64)
# entity BVHs: the one- and two-level forms and the generic walk (a depth-6 world: form 16 has no BVH instantiation), each with
# stacks short enough for 32 parked paths and tall enough to force 16 (the heights: tests/test_list_route_cpu.py)
for form, tree in ((16, -1), (17, 17), (18, 18)):
    for pool, leaf in BVH_LEAF.items():
        add(f"entities-form{form}-bvh{pool}-permuted-1337", ("entities", form, leaf), (tree, pool, True, False, False))
for form, tree in ((16, -1), (17, 17), (18, 18)):
    add(f"outdoor-form{form}-ext-permuted-1337", ("outdoor", form), (tree, 32, False, True, False), ext=EXT)
    add(f"entities-form{form}-extbvh-permuted-1337", ("entities", form, 4), (tree, 16, True, True, False), ext=EXT)
add("outdoor-form16-extsun-permuted-1337", ("outdoor", 16), (-1, 32, False, True, False), ext=dict(EXT, sun_sampling=1, emitters=0))
for opts in ((3, 2, 0.0), (40, 9, 2.5)):
    tag = f"depth{opts[0]}-{opts[1]}"
    add(f"outdoor-form16-{tag}-permuted-1337", ("outdoor", 16), plain(16), opts=opts)
    add(f"entities-form16-{tag}bvh-permuted-1337", ("entities", 16, 4), (-1, 32, True, False, False), opts=opts)
# ---- projected cameras x kind -------------------------------------------------------------------------------------------------------
add("outdoor-form16-fisheye+sorted-permuted-1337", ("outdoor", 16), (16, 64, False, False, True), proj="fisheye", variant=256)
add("entities-form16-panoramic+bvh-permuted-1337", ("entities", 16, 4), (-1, 32, True, False, False), proj="panoramic")
add("outdoor-form16-stereographic+ext-permuted-1337", ("outdoor", 16), (-1, 32, False, True, False), proj="stereographic", ext=EXT)
add("outdoor-form18-slot-permuted-1337", ("outdoor", 18), plain(18), proj="slot")
# ---- list shapes --------------------------------------------------------------------------------------------------------------------
for name in ("outdoor", "pregen"):
    for what, listed in shape_lists():
        add(f"{name}-form16-plain-{what}", (name, 16), plain(16), listed=listed)
    add(f"{name}-form16-plain-rowmajor-{NP}", (name, 16), plain(16), listed=whole_image(name))
    for n in PASS_COUNTS:
        add(f"{name}-form16-plain-permuted-257-{n}passes", (name, 16), plain(16), listed=pixel_list(257, "permuted"), passes=n)
# ---- launch splitting: 257 passes over a list of 5 pixels are two launches, of 256 passes and of 1 (tests/test_list_route_cpu.py) ----
for name in ("outdoor", "pregen"):
    add(f"{name}-form16-plain-permuted-{SPLIT_LIST}-{SPLIT_PASSES}passes", (name, 16), plain(16), listed=cell_list(3, SPLIT_LIST),
        passes=SPLIT_PASSES)

assert len({c.id for c in CELLS}) == len(CELLS)


def build(cell):
    if cell.scene == ("offset",):
        sc = gs.embedded_offset()
    elif cell.scene == ("any",):
        sc = gs.embedded_any()
    else:
        sc = scene(*cell.scene)
    if cell.ext:
        from test_gpu_extensions import with_spec_words
        sc = with_spec_words(sc)
    if cell.proj:
        from test_gpu_camera_projections import projected
        sc = projected(sc, PROJ[cell.proj])
    return sc


def oracle(port, cell, sc, seeds):
    """The oracle's image on the listed pixels (zero elsewhere)."""
    def render():
        if cell.proj:
            from test_gpu_camera_projections import equivalent
            return equivalent(port, sc, seeds, gids=cell.listed)
        return port.render_gids(sc, seeds, cell.listed)
    if cell.ext:
        with PortExt(port, sc, **cell.ext):
            return render()
    if cell.opts:
        with PortOptions(port, *cell.opts):
            return render()
    return render()


@pytest.mark.parametrize("cell", CELLS, ids=[c.id for c in CELLS])
def test_list(gpu_instance, port, cell):
    sc = build(cell)
    assert (sc.width, sc.height) == (gs.W, gs.H)
    seeds = SEEDS[:cell.passes]
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    r.set_option(native.OPT_KERNEL, cell.variant)
    for k, v in (cell.ext or {}).items():
        r.set_option(EXT_OPTS[k], v)
    if cell.opts:
        for k, v in zip((native.OPT_DRAW_DEPTH, native.OPT_MAX_DEPTH, native.OPT_EMITTER_SCALE), cell.opts):
            r.set_option(k, v)
    fb = torch.full((3 * NP,), MARKER, dtype=torch.float32, device="cuda")  # a caller-owned buffer holding the marker
    torch.cuda.synchronize()
    r.set_device_buffer(fb.data_ptr())
    r.render_list(cell.listed, seeds)
    info = r.kernel_info()
    got = r.read().reshape(NP, 3)
    r.set_device_buffer(None)
    r.close()
    loader.close()
    assert (info["tree"], info["pool"], info["bvh"], info["ext"], info["sorted"]) == cell.want, info
    want = oracle(port, cell, sc, seeds).reshape(NP, 3)
    same = (bits(got[cell.listed]) == bits(want[cell.listed])).all(axis=1)
    if not same.all():
        k = int(np.argmin(same))
        pytest.fail(f"{int((~same).sum())} of {same.size} listed pixels differ from the oracle (first: slot {k}, pixel {int(cell.listed[k])}: "
                    f"{got[cell.listed[k]].tolist()} against {want[cell.listed[k]].tolist()})")
    rest = np.ones(NP, bool)
    rest[cell.listed] = False
    kept = (bits(got[rest]) == bits(np.full(3, MARKER, np.float32))).all(axis=1)
    assert kept.all(), f"{int((~kept).sum())} pixels that are not listed were written (first: pixel {int(np.flatnonzero(rest)[np.argmin(kept)])})"
    if (cell.ext or cell.opts) and not cell.proj:  # the options changed the image: the cell did not compare two default renders
        base = port.render_gids(sc, seeds, cell.listed).reshape(NP, 3)
        assert not np.array_equal(bits(base[cell.listed]), bits(want[cell.listed])), "the options changed nothing on this scene"
