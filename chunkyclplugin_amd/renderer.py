"""Host-side mirror of the reference's device-binding layer, on top of the C ABI.

The reference's L2/L4 classes and their counterparts here:

=====================================================  ==========================================
reference (Java, JOCL)                                 this module (Python, ctypes -> libchunky_hip)
=====================================================  ==========================================
`RendererInstance.get()` (RendererInstance.java:23)    `RendererInstance.get(device)`
`ClSceneLoader` getters (ClSceneLoader.java:95-150)     `HipSceneLoader.load_packed(scene)` + getters
`ClCamera` (ClCamera.java:33-105)                       `HipPathTracingRenderer.set_camera`, `.set_lens`
`OpenClPathTracingRenderer.render` (:54-191)            `HipPathTracingRenderer.render`
`OpenClPreviewRenderer.render` (:47-115)                `HipPathTracingRenderer.preview`
=====================================================  ==========================================

What is NOT here: walking Chunky's `Scene` object (needs chunky-core; the Java side in
INTEGRATION.md does that and hands the same packed arrays to the same C entry points).
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Callable, Optional

import numpy as np

from . import native
from .native import check, ptr


def camera_rays(projector_type: int, settings, width: int, height: int, seed: int, lens=None) -> np.ndarray:
    """The projector type -1 table equivalent to a projected camera (types 1-5, 7, 8) in the pass of `seed`: feeding it to
    set_camera(-1, ...) renders that pass bit for bit (include/chunky_hip.h chunky_camera_rays).  lens = (aperture, focus): the
    table of that camera with the lens set_lens(aperture, focus) gives it (chunky_camera_rays_lens).  Host only."""
    return native.camera_rays(projector_type, settings, width, height, seed, lens)


def denoise_frame(instance, width: int, height: int, color, albedo, normal, params=None) -> np.ndarray:
    """chunky_denoise_frame: the A-Trous filter on `instance`'s device over host images (3 floats per pixel each); returns a
    (height, width, 3) float32 array equal, bit for bit, to native.denoise_host on the same inputs.  `params`: native.denoise_params()."""
    c, a, n = native._images(width, height, color, albedo, normal)
    p = params if params is not None else native.denoise_params()
    out = np.empty((int(height), int(width), 3), np.float32)
    check(native.lib().chunky_denoise_frame(instance._h, int(width), int(height), ptr(c), ptr(a), ptr(n), C.byref(p), ptr(out)))
    return out


class RendererInstance:
    """One GPU context per device index (the reference keeps a singleton for its one cl_device,
    RendererInstance.java:23-28; `clDevice` index from PersistentSettings :33)."""

    _instances = {}

    def __init__(self, device: int = 0):
        self.device = device
        self._h = C.c_void_p()
        check(native.lib().chunky_init(device, C.byref(self._h)))

    @classmethod
    def get(cls, device: int = 0) -> "RendererInstance":
        if device not in cls._instances:
            cls._instances[device] = RendererInstance(device)
        return cls._instances[device]

    @classmethod
    def group(cls, devices) -> "RendererInstance":
        """Several GPUs behind one context in this process (chunky_group_create): scenes are replicated, render targets
        are cut into 16 x 16-pixel blocks dealt round-robin to the members, `read()` gathers them on member 0.
        `devices` may repeat an index (members then share that GPU)."""
        self = cls.__new__(cls)
        self.device = int(devices[0])
        self.devices = [int(d) for d in devices]
        self._h = C.c_void_p()
        arr = (C.c_int * len(self.devices))(*self.devices)
        check(native.lib().chunky_group_create(arr, len(self.devices), C.byref(self._h)))
        return self

    def group_size(self) -> int:
        return native.lib().chunky_group_size(self._h)

    def peer_status(self) -> list:
        """chunky_group_peer_status: per member, how its share of a read-back reaches member 0 — native.PEER_LOCAL /
        PEER_DIRECT (xGMI) / PEER_STAGED, or a negated HIP error code when enabling peer access failed."""
        n = self.group_size()
        out = (C.c_int * n)()
        check(native.lib().chunky_group_peer_status(self._h, out, n))
        return list(out)

    TRANSPORT_NAMES = {native.TRANSPORT_PEER_COPY: "peer-copy", native.TRANSPORT_RCCL_SENDRECV: "rccl-sendrecv",
                       native.TRANSPORT_RCCL_REDUCE: "rccl-reduce"}

    def transport(self) -> dict:
        """chunky_group_transport: what carries the one exchange per read-back — {"transport": native.TRANSPORT_*, "name",
        "backend": "rccl" | "peer-copy", "detail": library / version / ranks, or the reason for the peer-copy fallback}."""
        t = C.c_int()
        buf = C.create_string_buffer(512)
        check(native.lib().chunky_group_transport(self._h, C.byref(t), buf, len(buf)))
        return {"transport": t.value, "name": self.TRANSPORT_NAMES.get(t.value, str(t.value)),
                "backend": "peer-copy" if t.value == native.TRANSPORT_PEER_COPY else "rccl",
                "detail": buf.value.decode("utf-8", "replace")}

    def set_transport(self, transport: int) -> None:
        """chunky_group_set_transport (ChunkyHipError with code E_STATE when it needs an RCCL communicator that is not there)."""
        check(native.lib().chunky_group_set_transport(self._h, int(transport)))

    @staticmethod
    def device_count() -> int:
        return native.lib().chunky_device_count()

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        check(native.lib().chunky_device_name(self.device, buf, 256))
        return buf.value.decode()

    def selftest_math(self, which: int, a, b=None) -> np.ndarray:
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(a if b is None else b, np.float32)
        out = np.empty_like(a)
        check(native.lib().chunky_selftest_math(self._h, which, a.size, ptr(a), ptr(b), ptr(out)))
        return out

    def selftest_shard_map(self, width: int, height: int, rank: int, world: int, tile: int, n_slots: int):
        """chunky_selftest_shard_map, mode 0: the device's slot -> pixel functions on the view set_shard would store.  Returns
        (rows (n_slots, 5) int32 = pool_slot_gid, pool_slot_pixel gid / x / y, shard_gid or -1; view = (rank, world, clamped tile, n_local))."""
        out = np.zeros((int(n_slots), 5), np.int32)
        view = np.zeros(4, np.int32)
        check(native.lib().chunky_selftest_shard_map(self._h, 0, width, height, rank, world, tile, int(n_slots), None, ptr(out), ptr(view)))
        return out, tuple(int(v) for v in view)

    def selftest_fast_quotient(self, n, d) -> np.ndarray:
        """chunky_selftest_shard_map, mode 1: n // d as the kernels divide by a launch constant (n < 2^31, d >= 1)."""
        pairs = np.ascontiguousarray(np.stack([np.asarray(n, np.uint32), np.asarray(d, np.uint32)], axis=1))
        out = np.zeros(len(pairs), np.int32)
        check(native.lib().chunky_selftest_shard_map(self._h, 1, 0, 0, 0, 1, 0, len(pairs), ptr(pairs), ptr(out), None))
        return out

    def selftest_gamma_scan(self, curve: int, first_bits: int, count: int):
        """(values whose tone-map byte differs from the threshold table's, worst stray of the estimate) over `count` float bit patterns."""
        bad, worst = C.c_uint64(0), C.c_float(0)
        check(native.lib().chunky_selftest_gamma_scan(self._h, curve, first_bits, count, C.byref(bad), C.byref(worst)))
        return int(bad.value), float(worst.value)

    def close(self) -> None:
        if self._h:
            check(native.lib().chunky_shutdown(self._h))
            self._h = C.c_void_p()
            if RendererInstance._instances.get(self.device) is self:
                RendererInstance._instances.pop(self.device, None)


class HipSceneLoader:
    """Device copies of one packed scene — the buffer side of `ClSceneLoader`.

    `load_packed` takes the arrays Chunky's packers produce (here: `scenes.PackedScene`) and uploads
    them through the same entry points the JNI layer binds."""

    def __init__(self, instance: Optional[RendererInstance] = None):
        self.instance = instance or RendererInstance.get()
        self._h = C.c_void_p()
        check(native.lib().chunky_scene_create(self.instance._h, C.byref(self._h)))
        self.packed = None
        self._has_biome = False

    def load_packed(self, sc) -> bool:
        L = native.lib()
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        tree = i32(sc.octree)
        check(L.chunky_scene_set_octree(self._h, ptr(tree), tree.size, int(sc.octree_depth)))
        for kind, arr in ((native.PALETTE_BLOCK, sc.block_palette), (native.PALETTE_MATERIAL, sc.material_palette),
                          (native.PALETTE_AABB, sc.aabb_models), (native.PALETTE_QUAD, sc.quad_models),
                          (native.PALETTE_TRIG, sc.bvh_trigs)):
            a = i32(arr)
            check(L.chunky_scene_set_palette(self._h, kind, ptr(a), a.size))
        for which, arr in ((native.BVH_WORLD, sc.world_bvh), (native.BVH_ACTOR, sc.actor_bvh)):
            a = i32(arr)
            check(L.chunky_scene_set_bvh(self._h, which, ptr(a), a.size))
        atlas = np.ascontiguousarray(sc.atlas, np.uint8)
        layers, h, w, _ = atlas.shape
        check(L.chunky_scene_set_atlas(self._h, ptr(atlas), w, h, layers))
        sky = np.ascontiguousarray(sc.sky, np.uint8)
        check(L.chunky_scene_set_sky(self._h, ptr(sky), sky.shape[1], sky.shape[0], float(sc.sky_intensity)))
        sun = i32(sc.sun)
        check(L.chunky_scene_set_sun(self._h, ptr(sun)))
        biome = getattr(sc, "biome", None)
        if biome is not None:
            self.set_biome_tints(*biome)
        elif self._has_biome:  # the scene loaded before had a map, this one has none
            self.set_biome_tints(0, 0, None)
        self.packed = sc
        return True

    def set_biome_tints(self, x0: int, z0: int, rgb) -> None:
        """chunky_scene_set_biome_tints: rgb[size_z, size_x, 3] holds the foliage, grass and water colour (RGB in the low 24 bits) of
        the octree cells x0 <= x < x0 + size_x, z0 <= z < z0 + size_z; rgb = None removes the map."""
        if rgb is None:
            check(native.lib().chunky_scene_set_biome_tints(self._h, None, 0, 0, 0, 0))
            self._has_biome = False
            return
        a = np.ascontiguousarray(rgb, np.int32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"expected colours of shape (size_z, size_x, 3), got {a.shape}")
        check(native.lib().chunky_scene_set_biome_tints(self._h, ptr(a), int(x0), int(z0), a.shape[1], a.shape[0]))
        self._has_biome = True

    def emitters(self) -> np.ndarray:
        """The emitter list of the next-event-estimation extension: rows {x, y, z, level << 25 | block pointer}."""
        n = C.c_int32()
        check(native.lib().chunky_scene_emitters(self._h, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 4), np.int32)
        check(native.lib().chunky_scene_emitters(self._h, ptr(out), n.value, C.byref(n)))
        return out[:n.value]

    def addr32(self) -> int:
        """chunky_scene_addr32: the arrays the next launch reads by 32-bit offsets (native.ADDR32_*)."""
        word = C.c_uint32()
        check(native.lib().chunky_scene_addr32(self._h, C.byref(word)))
        return word.value

    def hit_top(self) -> int:
        """chunky_scene_hit_top: 1 + the highest cell y of any leaf that can be hit, as the next launch carries it."""
        top = C.c_int32()
        check(native.lib().chunky_scene_hit_top(self._h, C.byref(top)))
        return top.value

    def selftest_helpers(self, which: int, rows, tree: int = 1):
        """chunky_selftest_helpers: the device counterpart of reference helper `which` on rows of 32 floats; returns
        (rows of 12 floats, tree form used for row kind 14)."""
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 32)
        out = np.zeros((len(rows), 12), np.float32)
        used = C.c_int32()
        check(native.lib().chunky_selftest_helpers(self._h, which, tree, len(rows), ptr(rows), ptr(out), C.byref(used)))
        return out, used.value

    def load_octree(self, tree_data, depth: int, block_mapping) -> None:
        """`ClSceneLoader.loadOctree` (ClSceneLoader.java:52-63): raw PackedOctree.treeData +
        blockMapping, remapped natively."""
        t = np.ascontiguousarray(tree_data, np.int32)
        m = np.ascontiguousarray(block_mapping, np.int32)
        check(native.lib().chunky_scene_load_octree(self._h, ptr(t), t.size, depth, ptr(m), m.size))

    def close(self) -> None:
        if self._h:
            check(native.lib().chunky_scene_destroy(self._h))
            self._h = C.c_void_p()


class HipPathTracingRenderer:
    """`OpenClPathTracingRenderer` for one image: ids, pass loop, read-back and merge."""

    ID = "ChunkyClRenderer"  # OpenClPathTracingRenderer.java:33-46 (getId/getName/getDescription)

    def __init__(self, scene_loader: HipSceneLoader, width: int, height: int):
        self.scene_loader = scene_loader
        self.width, self.height = width, height
        self._h = C.c_void_p()
        self.post_render: Optional[Callable[[], bool]] = None
        check(native.lib().chunky_render_create(scene_loader.instance._h, scene_loader._h, width, height,
                                                C.byref(self._h)))

    # --- Renderer interface -----------------------------------------------------------------
    def get_id(self) -> str:
        return self.ID

    def set_post_render(self, callback: Optional[Callable[[], bool]]) -> None:
        self.post_render = callback

    def auto_post_process(self) -> bool:
        return False  # OpenClPathTracingRenderer.java:197-200

    # --- camera / options -------------------------------------------------------------------
    def set_camera(self, projector_type: int, settings) -> None:
        s = np.ascontiguousarray(settings, np.float32)
        check(native.lib().chunky_render_set_camera(self._h, int(projector_type), ptr(s), s.size))

    def set_lens(self, aperture: float, focus: float) -> None:
        """chunky_render_set_lens: depth of field for the projected camera set last (types 1-5, 7, 8): a lens disc of radius
        `aperture` in focus at distance `focus`; aperture 0 switches it off.  set_camera clears the lens."""
        check(native.lib().chunky_render_set_lens(self._h, float(aperture), float(focus)))

    def set_canvas(self, canvas_width: int, canvas_height: int, x0: int = 0, y0: int = 0) -> None:
        """chunky_render_set_canvas: this target is the window at (x0, y0) of a canvas_width x canvas_height canvas — it stores, per
        pixel, exactly what a target of the canvas's size stores at that canvas pixel.  canvas == target at (0, 0) switches the
        window off.  It touches no image: reset() (and the other passes' resets) before rendering another window."""
        check(native.lib().chunky_render_set_canvas(self._h, int(canvas_width), int(canvas_height), int(x0), int(y0)))

    def canvas(self):
        """chunky_render_canvas: (canvas_width, canvas_height, x0, y0)."""
        out = np.zeros(4, np.int32)
        check(native.lib().chunky_render_canvas(self._h, ptr(out)))
        return tuple(int(v) for v in out)

    def set_fog(self, density: float, y_min: float = 0.0, y_max: float = 1.0, color=(1.0, 1.0, 1.0)) -> None:
        """chunky_render_set_fog: a homogeneous, isotropically scattering fog layer of `density` per block between the heights y_min
        and y_max (octree coordinates) with single-scattering colour `color`, path traced by render_passes.  density 0 turns it off.
        It touches no image: reset() before rendering with another layer."""
        if float(density) == 0.0:
            check(native.lib().chunky_render_set_fog(self._h, None))
        else:
            check(native.lib().chunky_render_set_fog(self._h, C.byref(native.fog_struct(density, y_min, y_max, color))))

    def fog(self) -> dict:
        """chunky_render_fog: the target's fog layer (density 0: none)."""
        f = native.Fog()
        f.size = C.sizeof(native.Fog)
        check(native.lib().chunky_render_fog(self._h, C.byref(f)))
        return {"density": float(f.density), "y_min": float(f.y_min), "y_max": float(f.y_max), "color": tuple(float(c) for c in f.color)}

    def set_translucency(self, opaque_alpha: Optional[float] = 0.99, max_crossings: int = 8) -> None:
        """chunky_render_set_translucency: hits whose alpha (after the tint) is below `opaque_alpha` let light through — a path's ray
        crosses with probability 1 - alpha, a shadow ray is filtered — at most `max_crossings` times per ray.
        opaque_alpha None turns the feature off.  It touches no image: reset() before rendering with another setting."""
        if opaque_alpha is None:
            check(native.lib().chunky_render_set_translucency(self._h, None))
        else:
            check(native.lib().chunky_render_set_translucency(self._h, C.byref(native.translucency_struct(opaque_alpha, max_crossings))))

    def translucency(self) -> dict:
        """chunky_render_translucency: the target's setting."""
        t = native.Translucency()
        t.size = C.sizeof(native.Translucency)
        on = C.c_int(0)
        check(native.lib().chunky_render_translucency(self._h, C.byref(t), C.byref(on)))
        return {"enabled": bool(on.value), "opaque_alpha": float(t.opaque_alpha), "max_crossings": int(t.max_crossings)}

    def camera_rays(self, seed: int) -> np.ndarray:
        """Self test of a projected camera (types 1-5, 7, 8, with its lens if one is set): the rays the render kernels compute for the pass of `seed`, every pixel,
        width*height*6 floats as camera_rays() lays them out."""
        out = np.zeros(self.width * self.height * 6, np.float32)
        check(native.lib().chunky_selftest_camera_rays(self._h, int(np.int32(np.uint32(int(seed) & 0xFFFFFFFF))), ptr(out), out.size))
        return out

    def set_option(self, option: int, value) -> None:
        if option == native.OPT_EMITTER_SCALE:
            value = struct.unpack("<i", struct.pack("<f", float(value)))[0]
        check(native.lib().chunky_render_set_option(self._h, option, int(value)))

    def set_shard(self, rank: int, world: int, tile: int = 256) -> None:
        check(native.lib().chunky_render_set_shard(self._h, rank, world, tile))

    def set_device_buffer(self, device_ptr: Optional[int]) -> None:
        check(native.lib().chunky_render_set_device_buffer(self._h, device_ptr))

    def device_buffer(self) -> int:
        p = C.c_void_p()
        check(native.lib().chunky_render_device_buffer(self._h, C.byref(p)))
        return p.value

    # --- passes -------------------------------------------------------------------------------
    def reset(self) -> None:
        check(native.lib().chunky_render_reset(self._h))

    def render_passes(self, seeds, first_buffer_spp: int = 0, sync: bool = True) -> None:
        s = np.ascontiguousarray(seeds, np.int32)
        check(native.lib().chunky_render_passes(self._h, ptr(s), s.size, first_buffer_spp))
        if sync:
            self.sync()

    def sync(self) -> None:
        check(native.lib().chunky_render_sync(self._h))

    def gather(self) -> None:
        """The read-back exchange without the copy to the host (a group: member 0's device buffer then holds the image)."""
        check(native.lib().chunky_render_gather(self._h))

    def read(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """chunky_render_read (on a group: the one exchange, then the copy); `out` = a float32 array to fill — e.g. pinned memory."""
        if out is None:
            out = np.empty(self.width * self.height * 3, np.float32)
        assert out.dtype == np.float32 and out.size == self.width * self.height * 3 and out.flags["C_CONTIGUOUS"]
        check(native.lib().chunky_render_read(self._h, ptr(out), out.size))
        return out

    def kernel_time(self):
        ms, n = C.c_float(), C.c_int()
        check(native.lib().chunky_render_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_info(self) -> dict:
        """The kernel instantiation the last launch ran: tree form, lanes per pixel, entity-BVH phases, workgroups."""
        out = np.zeros(8, np.int32)
        check(native.lib().chunky_render_kernel_info(self._h, ptr(out)))
        return {"tree": int(out[0]), "group": int(out[1]), "bvh": bool(out[2]), "blocks": int(out[3]), "pool": int(out[4]),
                "ext": int(out[5]) == 1, "biome": int(out[5]) == native.KERNEL_BIOME, "fog": int(out[5]) == native.KERNEL_FOG, "glass": int(out[5]) == native.KERNEL_GLASS,
                "passes_per_launch": int(out[6]), "sorted": bool(out[7])}

    def phase_stats(self, reset: bool = True) -> dict:
        out = np.zeros(24, np.uint64)
        check(native.lib().chunky_render_phase_stats(self._h, ptr(out), 1 if reset else 0))
        o = out[:9].reshape(3, 3)
        d = {name: {"execs": int(o[i, 0]), "lanes": int(o[i, 1]), "cycles": int(o[i, 2])}
             for i, name in enumerate(("march", "block", "shade"))}
        d["waves"] = {"life_sum": int(out[9]), "life_max": int(out[10]), "n": int(out[11])}
        d["handover"] = {"execs": int(out[12]), "cycles": int(out[13])}
        d["parts"] = {name: int(out[14 + i]) for i, name in enumerate(
            ("sky", "sampling", "trace_setup", "deposit", "fold", "open_pixel", "hand_out", "new_sample"))}
        # render_pool's sorted instantiation: the model blocks' phase ("block" is then the full cubes alone)
        d["model"] = {"execs": int(out[22]) >> 40, "lanes": int(out[22]) & ((1 << 40) - 1), "cycles": int(out[23])}
        return d

    def march_above(self, reset: bool = True) -> int:
        """chunky_render_march_above: of the march lanes of phase_stats, the lane-steps of upward rays at or above hit_top."""
        out = np.zeros(1, np.uint64)
        check(native.lib().chunky_render_march_above(self._h, ptr(out), 1 if reset else 0))
        return int(out[0])

    def preview(self) -> np.ndarray:
        out = np.empty(self.width * self.height, np.int32)
        check(native.lib().chunky_render_preview(self._h, ptr(out)))
        return out

    def trace_records(self, seed: int, gids):
        g = np.ascontiguousarray(gids, np.int32)
        rec = np.zeros((g.size, native.MAX_TRACES), native.HIT_DTYPE)
        cnt = np.zeros(g.size, np.int32)
        rad = np.zeros((g.size, 3), np.float32)
        check(native.lib().chunky_render_trace_records(self._h, int(seed), ptr(g), g.size, ptr(rec), ptr(cnt), ptr(rad)))
        return rec, cnt, rad

    # --- auxiliary images for a denoiser (chunky_render_aov_*) ---------------------------------------
    def render_aov(self, seeds, first_buffer_spp: int = 0, sync: bool = True) -> None:
        """Albedo and normal passes: pass k uses seeds[k] and bufferSpp first_buffer_spp + k, like render_passes, and traces the
        first ray of that render pass only."""
        s = np.ascontiguousarray(seeds, np.int32)
        check(native.lib().chunky_render_aov_passes(self._h, ptr(s), s.size, first_buffer_spp))
        if sync:
            self.sync()

    def read_aov(self, which: int) -> np.ndarray:
        """One AOV image (native.AOV_ALBEDO or native.AOV_NORMAL) as a (height, width, 3) float32 array."""
        out = np.empty((self.height, self.width, 3), np.float32)
        check(native.lib().chunky_render_aov_read(self._h, int(which), ptr(out), out.size))
        return out

    def reset_aov(self) -> None:
        check(native.lib().chunky_render_aov_reset(self._h))

    def aov_kernel_time(self):
        """(milliseconds, launches) of the AOV kernel since the last call."""
        ms, n = C.c_float(), C.c_int()
        check(native.lib().chunky_render_aov_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def aov_info(self) -> dict:
        """The AOV instantiation the last AOV launch ran: tree form, entity-BVH walk, workgroups, launches of the last call."""
        out = np.zeros(4, np.int32)
        check(native.lib().chunky_render_aov_kernel_info(self._h, ptr(out)))
        return {"tree": int(out[0]), "bvh": bool(out[1] & 1), "biome": bool(out[1] & native.KERNEL_BIOME), "blocks": int(out[2]), "launches": int(out[3])}

    # --- the first-hit images beside them (chunky_render_aov_passes_ex / _read_ex) -------------------
    def render_aov_ex(self, seeds, first_buffer_spp: int = 0, sync: bool = True) -> None:
        """render_aov with coverage, depth, position, emittance and block id folded from the same trace (all seven images)."""
        s = np.ascontiguousarray(seeds, np.int32)
        check(native.lib().chunky_render_aov_passes_ex(self._h, ptr(s), s.size, first_buffer_spp))
        if sync:
            self.sync()

    def read_aov_ex(self, which: int) -> np.ndarray:
        """One of the seven images (native.AOV_ALBEDO .. native.AOV_BLOCK): (height, width, 3) float32 for albedo, normal and
        position, (height, width) float32 for alpha, depth and emittance, (height, width) int32 for the block id."""
        words = native.AOV_WORDS.get(int(which), 1)  # (an unknown image: the library refuses it)
        shape = (self.height, self.width, 3) if words == 3 else (self.height, self.width)
        out = np.empty(shape, np.int32 if which == native.AOV_BLOCK else np.float32)
        check(native.lib().chunky_render_aov_read_ex(self._h, int(which), ptr(out), out.size))
        return out

    # --- sun shadow and ambient occlusion of the beauty sample's rays (chunky_render_occlusion_*) ------
    def render_occlusion(self, seeds, ao_distance: float, first_buffer_spp: int = 0, sync: bool = True) -> None:
        """Occlusion passes: pass k follows the render pass with seeds[k] through its sun ray and its first bounce ray and folds "the sun
        ray was free" and "the bounce ray met nothing within ao_distance" (> 0; inf allowed) into two images."""
        s = np.ascontiguousarray(seeds, np.int32)
        check(native.lib().chunky_render_occlusion_passes(self._h, ptr(s), s.size, first_buffer_spp, float(ao_distance)))
        if sync:
            self.sync()

    def read_occlusion(self, which: int) -> np.ndarray:
        """One of the two images (native.AOV_AO or native.AOV_SUN) as a (height, width) float32 array."""
        out = np.empty((self.height, self.width), np.float32)
        check(native.lib().chunky_render_occlusion_read(self._h, int(which), ptr(out), out.size))
        return out

    def reset_occlusion(self) -> None:
        check(native.lib().chunky_render_occlusion_reset(self._h))

    def occlusion_time(self):
        """(milliseconds, launches) of the occlusion kernel since the last call."""
        ms, n = C.c_float(), C.c_int()
        check(native.lib().chunky_render_occlusion_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def occlusion_info(self) -> dict:
        """The instantiation the last occlusion launch ran: tree form, entity-BVH walk, workgroups, launches of the last call."""
        out = np.zeros(4, np.int32)
        check(native.lib().chunky_render_occlusion_kernel_info(self._h, ptr(out)))
        return {"tree": int(out[0]), "bvh": bool(out[1]), "blocks": int(out[2]), "launches": int(out[3])}

    # --- light groups: the sky's, the sun's and the emitters' share of the beauty image (chunky_render_light_*) ------
    def render_lights(self, seeds, first_buffer_spp: int = 0, sync: bool = True) -> None:
        """Light-group passes: pass k walks the path of the render pass with seeds[k] once and folds its radiance into four images —
        the sky's, the sun's and the emitters' share, and their sum as the beauty pass adds it."""
        s = np.ascontiguousarray(seeds, np.int32)
        check(native.lib().chunky_render_light_passes(self._h, ptr(s), s.size, first_buffer_spp))
        if sync:
            self.sync()

    def read_light(self, which: int) -> np.ndarray:
        """One of the four images (native.LIGHT_SKY, _SUN, _EMITTERS, _ALL) as a (height, width, 3) float32 array."""
        out = np.empty((self.height, self.width, 3), np.float32)
        check(native.lib().chunky_render_light_read(self._h, int(which), ptr(out), out.size))
        return out

    def mix_lights(self, weights) -> np.ndarray:
        """(w0 * SKY + w1 * SUN) + w2 * EMITTERS, mixed on the device, as a (height, width, 3) float32 array."""
        w = np.ascontiguousarray(weights, np.float32)
        if w.shape != (3,):
            raise ValueError("mix_lights takes three weights: sky, sun, emitters")
        out = np.empty((self.height, self.width, 3), np.float32)
        check(native.lib().chunky_render_light_mix(self._h, ptr(w), ptr(out), out.size))
        return out

    def reset_lights(self) -> None:
        check(native.lib().chunky_render_light_reset(self._h))

    def lights_time(self):
        """(milliseconds, launches) of the light-group kernel since the last call."""
        ms, n = C.c_float(), C.c_int()
        check(native.lib().chunky_render_light_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def lights_info(self) -> dict:
        """The instantiation the last light-group launch ran: tree form, entity-BVH walk, whether it carried the emitter groups, workgroups,
        launches of the last call."""
        out = np.zeros(4, np.int32)
        check(native.lib().chunky_render_light_kernel_info(self._h, ptr(out)))
        return {"tree": int(out[0]), "bvh": bool(out[1] & 1), "groups": bool(out[1] & native.KERNEL_LIGHT_GROUPS), "blocks": int(out[2]),
                "launches": int(out[3])}

    def set_emitter_groups(self, mapping, n_groups: Optional[int] = None) -> int:
        """Split the emitters' share by what emits: `mapping` is {id: group} over block pointers (scenes.emitter_ids),
        native.MATTE_WORLD_ENTITY and native.MATTE_ACTOR_ENTITY; every other id is group 0.  n_groups defaults to the highest group
        named + 1; an empty mapping with n_groups None (or 0) drops the groups.  The group images start at zero and the four images
        are not touched: call reset_lights() too unless they are empty.  Returns the number of groups."""
        ids = np.array(list(mapping.keys()), np.int32)
        groups = np.array([int(mapping[k]) for k in mapping], np.int64)
        if len(groups) and (groups.min() < 0 or groups.max() > 255):
            raise ValueError("a group is a number from 0 to 255")
        n = int(groups.max()) + 1 if n_groups is None and len(groups) else int(n_groups or 0)
        g8 = groups.astype(np.uint8)
        check(native.lib().chunky_render_light_set_emitter_groups(self._h, n, ptr(ids) if len(ids) else None, ptr(g8) if len(ids) else None, len(ids)))
        return n

    def read_light_group(self, group: int) -> np.ndarray:
        """The image of one emitter group as a (height, width, 3) float32 array."""
        out = np.empty((self.height, self.width, 3), np.float32)
        check(native.lib().chunky_render_light_read_group(self._h, int(group), ptr(out), out.size))
        return out

    def mix_light_groups(self, w_sky: float, w_sun: float, w_groups) -> np.ndarray:
        """((w_sky * SKY + w_sun * SUN) + w_groups[0] * G0) + w_groups[1] * G1 ..., mixed on the device, as a (height, width, 3)
        float32 array; one weight per group of the target."""
        w = np.ascontiguousarray(w_groups, np.float32).reshape(-1)
        out = np.empty((self.height, self.width, 3), np.float32)
        check(native.lib().chunky_render_light_mix_groups(self._h, float(w_sky), float(w_sun), ptr(w) if w.size else None, w.size, ptr(out), out.size))
        return out

    # --- antialiased ID mattes (chunky_render_matte_*) ------------------------------------------------
    def render_matte(self, seeds, sync: bool = True) -> None:
        """Matte passes: pass k traces the first ray of the render pass with seeds[k] and counts the id it hits, per pixel."""
        s = np.ascontiguousarray(seeds, np.int32)
        check(native.lib().chunky_render_matte_passes(self._h, ptr(s), s.size))
        if sync:
            self.sync()

    def read_matte(self):
        """The matte state: (ids (6, height, width) int32, counts (6, height, width) int32, other (height, width) int32, passes)."""
        shape = (native.MATTE_SLOTS, self.height, self.width)
        ids, counts, other = np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape[1:], np.int32)
        passes = C.c_int32()
        check(native.lib().chunky_render_matte_read(self._h, ptr(ids), ptr(counts), ptr(other), other.size, C.byref(passes)))
        return ids, counts, other, passes.value

    def restore_matte(self, ids, counts, other, passes: int) -> None:
        """Replaces the matte state with one read_matte returned (a resumed render); a malformed state is refused and nothing changes."""
        i, c, o = (np.ascontiguousarray(a, np.int32) for a in (ids, counts, other))
        if i.size != native.MATTE_SLOTS * o.size or c.size != i.size:
            raise ValueError(f"expected ids and counts of {native.MATTE_SLOTS} planes of other's size, got {i.shape}, {c.shape}, {o.shape}")
        check(native.lib().chunky_render_matte_restore(self._h, ptr(i), ptr(c), ptr(o), o.size, int(passes)))

    def matte_ranks(self):
        """(ids (6, height, width) int32, coverage (6, height, width) float32): per pixel the ids by share of the passes, descending;
        empty ranks hold native.MATTE_EMPTY and 0."""
        shape = (native.MATTE_SLOTS, self.height, self.width)
        ids, cov = np.empty(shape, np.int32), np.empty(shape, np.float32)
        check(native.lib().chunky_render_matte_ranks(self._h, ptr(ids), ptr(cov), self.width * self.height))
        return ids, cov

    def matte_extract(self, id_set) -> np.ndarray:
        """The (height, width) float32 mask of a set of ids: the share of each pixel's passes that saw one of them — what
        HipPostProcessingFilter.process_frame_alpha takes as alpha."""
        st = np.ascontiguousarray(id_set, np.int32).reshape(-1)
        out = np.empty((self.height, self.width), np.float32)
        check(native.lib().chunky_render_matte_extract(self._h, ptr(st) if st.size else None, st.size, ptr(out), out.size))
        return out

    def reset_matte(self) -> None:
        check(native.lib().chunky_render_matte_reset(self._h))

    def matte_kernel_time(self):
        """(milliseconds, launches) of the matte-pass kernel since the last call."""
        ms, n = C.c_float(), C.c_int()
        check(native.lib().chunky_render_matte_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def matte_info(self) -> dict:
        """The instantiation the last matte launch ran: tree form, entity-BVH walk, workgroups, launches of the last call."""
        out = np.zeros(4, np.int32)
        check(native.lib().chunky_render_matte_kernel_info(self._h, ptr(out)))
        return {"tree": int(out[0]), "bvh": bool(out[1]), "blocks": int(out[2]), "launches": int(out[3])}

    # --- denoising (chunky_render_denoise) ------------------------------------------------------------
    def denoise(self, params=None) -> np.ndarray:
        """The framebuffer filtered with this target's AOV images, all on the device; only the (height, width, 3) result is read
        back.  Needs render_aov first; the framebuffer and the AOV images are left as they are."""
        p = params if params is not None else native.denoise_params()
        out = np.empty((self.height, self.width, 3), np.float32)
        check(native.lib().chunky_render_denoise(self._h, C.byref(p), ptr(out), out.size))
        return out

    def denoise_kernel_time(self):
        """(milliseconds, launches) of the denoise kernels since the last call."""
        ms, n = C.c_float(), C.c_int()
        check(native.lib().chunky_render_denoise_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # --- adaptive sampling (chunky_render_adaptive) ---------------------------------------------------
    def render_adaptive(self, seeds, params=None):
        """Renders until every pixel's noise estimate is under params.threshold or len(seeds) passes are done (blocking; resets the
        target first).  Returns (image (h, w, 3), counts (h, w) int32, noise (h, w, 2) = Welford (m, M2) of luminance, summary dict)."""
        s = np.ascontiguousarray(seeds, np.int32)
        p = params if params is not None else native.adaptive_params()
        summ = native.AdaptiveSummary()
        check(native.lib().chunky_render_adaptive(self._h, ptr(s), s.size, C.byref(p), C.byref(summ)))
        image = self.read().reshape(self.height, self.width, 3)
        summary = native.adaptive_summary_dict(summ)
        return image, self.adaptive_counts(), self.adaptive_noise(), summary

    def _adaptive_callbacks(self, post_render, round_done):
        """(struct or None, the ctypes thunks to keep alive during the call)"""
        if post_render is None and round_done is None:
            return None, ()
        cb = native.AdaptiveCallbacks()
        cb.struct_size = C.sizeof(native.AdaptiveCallbacks)
        keep = []
        if post_render is not None:
            keep.append(native.POST_RENDER_FN(lambda _u: 1 if post_render() else 0))
            cb.post_render = keep[-1]
        if round_done is not None:
            keep.append(native.ROUND_DONE_FN(lambda _u, passes, active: round_done(int(passes), int(active))))
            cb.round_done = keep[-1]
        return cb, keep

    def _adaptive_call(self, fn, seeds, params, post_render, round_done):
        s = np.ascontiguousarray(seeds, np.int32)
        p = params if params is not None else native.adaptive_params()
        summ = native.AdaptiveSummary()
        cb, keep = self._adaptive_callbacks(post_render, round_done)
        rc = fn(self._h, ptr(s), s.size, C.byref(p), C.byref(cb) if cb is not None else None, C.byref(summ))
        del keep
        if rc not in (0, native.E_ABORTED):
            check(rc)
        return rc == 0, native.adaptive_summary_dict(summ)

    def render_adaptive_ex(self, seeds, params=None, post_render=None, round_done=None):
        """chunky_render_adaptive_ex: render_adaptive from pass 0 with the hooks.  post_render() -> truthy stops the run at the next
        launch boundary; round_done(passes, active) is told of every round.  Neither may call into this instance's targets.  Returns
        (finished, summary): finished is False when post_render stopped the run — the target then holds a state that resume_adaptive
        continues, and read / adaptive_counts / adaptive_noise show the passes done."""
        return self._adaptive_call(native.lib().chunky_render_adaptive_ex, seeds, params, post_render, round_done)

    def resume_adaptive(self, seeds, params=None, post_render=None, round_done=None):
        """chunky_render_adaptive_resume: continues the target's adaptive state to len(seeds) passes.  `seeds` is the whole stream
        from pass 0 (the passes already done are skipped), `params` the parameters of the run being continued.  Returns (finished,
        summary), the summary counted from pass 0."""
        return self._adaptive_call(native.lib().chunky_render_adaptive_resume, seeds, params, post_render, round_done)

    def adaptive_state(self) -> "native.AdaptiveRun":
        """The target's whole adaptive state on the host (chunky_render_adaptive_state plus the readers): what restore_adaptive takes."""
        st = native.AdaptiveState()
        st.size = C.sizeof(native.AdaptiveState)
        active = np.empty((self.height, self.width), np.uint8)
        check(native.lib().chunky_render_adaptive_state(self._h, C.byref(st), ptr(active), active.size))
        return native.AdaptiveRun(st, self.read(), self.adaptive_counts(), self.adaptive_noise(), active)

    def restore_adaptive(self, run: "native.AdaptiveRun") -> None:
        """chunky_render_adaptive_restore: takes a state (of this target's size) onto the target; resume_adaptive continues it."""
        check(native.lib().chunky_render_adaptive_restore(self._h, C.byref(run.state), ptr(run.mean), ptr(run.count), ptr(run.stat), ptr(run.active)))

    def adaptive_counts(self) -> np.ndarray:
        out = np.empty((self.height, self.width), np.int32)
        check(native.lib().chunky_render_adaptive_counts(self._h, ptr(out), out.size))
        return out

    def adaptive_noise(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 2), np.float32)
        check(native.lib().chunky_render_adaptive_noise(self._h, ptr(out), out.size))
        return out

    def adaptive_kernel_time(self):
        """(milliseconds, rounds) of the adaptive runs since the last call: render launches, folds, checks and compactions."""
        ms, n = C.c_float(), C.c_int()
        check(native.lib().chunky_render_adaptive_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # --- firefly-robust accumulation (chunky_render_robust_*) -----------------------------------------
    def robust_begin(self, n_buckets: int) -> None:
        """chunky_render_robust_begin: n_buckets zeroed bucket images and a sample count of 0 (0 releases the state)."""
        check(native.lib().chunky_render_robust_begin(self._h, int(n_buckets)))

    def robust_passes(self, seeds, first_buffer_spp: int = 0, sync: bool = True) -> None:
        """chunky_render_robust_passes: render_passes plus the bucket fold of the same samples."""
        s = np.ascontiguousarray(seeds, np.int32)
        check(native.lib().chunky_render_robust_passes(self._h, ptr(s) if s.size else None, s.size, int(first_buffer_spp)))
        if sync:
            self.sync()

    def robust_bucket(self, b: int):
        """(bucket image (h, w, 3), robust sample count)"""
        out = np.empty((self.height, self.width, 3), np.float32)
        n = C.c_int32()
        check(native.lib().chunky_render_robust_read_bucket(self._h, int(b), ptr(out), out.size, C.byref(n)))
        return out, n.value

    def robust_buckets(self, n_buckets: int) -> np.ndarray:
        """All bucket images, (n_buckets, h, w, 3)."""
        return np.stack([self.robust_bucket(b)[0] for b in range(n_buckets)])

    def robust_resolve(self, params=None, trim: bool = True):
        """chunky_render_robust_resolve: (image (h, w, 3), trim (h, w) uint8 or None), resolved on the device."""
        p = params if params is not None else native.robust_params()
        out = np.empty((self.height, self.width, 3), np.float32)
        t = np.empty((self.height, self.width), np.uint8) if trim else None
        check(native.lib().chunky_render_robust_resolve(self._h, C.byref(p), ptr(out), out.size, ptr(t) if trim else None, t.size if trim else 0))
        return out, t

    def robust_denoise(self, params=None, denoise_params=None) -> np.ndarray:
        """chunky_render_robust_denoise: the resolved image filtered with this target's AOV images, all on the device."""
        p = params if params is not None else native.robust_params()
        d = denoise_params if denoise_params is not None else native.denoise_params()
        out = np.empty((self.height, self.width, 3), np.float32)
        check(native.lib().chunky_render_robust_denoise(self._h, C.byref(p), C.byref(d), ptr(out), out.size))
        return out

    def robust_kernel_time(self):
        """(milliseconds of the robust_passes launches, their number, milliseconds of the resolve kernels) since the last call."""
        ms, n, rs = C.c_float(), C.c_int(), C.c_float()
        check(native.lib().chunky_render_robust_kernel_time(self._h, C.byref(ms), C.byref(n), C.byref(rs)))
        return ms.value, n.value, rs.value

    def render_robust(self, seeds, n_buckets: int = 9, params=None, first_buffer_spp: int = 0):
        """Begins a robust state of n_buckets buckets, renders len(seeds) passes into it and the framebuffer, and resolves.  Returns
        (resolved image (h, w, 3), trim (h, w) uint8).  The resolved image is a biased estimator (it darkens rare bright paths with
        the fireflies); read() still returns the unbiased running mean of the same passes."""
        self.robust_begin(n_buckets)
        self.robust_passes(seeds, first_buffer_spp)
        return self.robust_resolve(params)

    def render_list(self, pixels, seeds) -> None:
        """chunky_selftest_render_list: len(seeds) passes on the listed pixel indices only, through the list route of the adaptive rounds."""
        px = np.ascontiguousarray(pixels, np.int32)
        s = np.ascontiguousarray(seeds, np.int32)
        check(native.lib().chunky_selftest_render_list(self._h, ptr(px), px.size, ptr(s), s.size))

    def render(self, sample_buffer: np.ndarray, scene_spp: int, target_spp: int, merge_interval: int = 1024) -> int:
        """The pass loop of OpenClPathTracingRenderer.render (:95-184) run natively; merges into the
        caller's double sample buffer and returns the new scene.spp."""
        assert sample_buffer.dtype == np.float64 and sample_buffer.size == self.width * self.height * 3
        spp = C.c_int32(scene_spp)
        cb = native.POST_RENDER_FN((lambda _u: 1 if self.post_render() else 0) if self.post_render else 0)
        rc = native.lib().chunky_render_run(self._h, ptr(sample_buffer), C.byref(spp), target_spp, merge_interval, cb, None)
        if rc not in (0, native.E_ABORTED):
            check(rc)
        return spp.value

    def render_ex(self, sample_buffer: np.ndarray, scene_spp: int, target_spp: int, merge_interval: int = 1024,
                  progress=None, merged=None, save_event=None, regenerate_camera=None, poll_gate=None) -> int:
        """chunky_render_run_ex: the same loop with the reference's other hooks — `progress(spp)` after every launch
        (scene.spp, :144), `merged(spp)` after every merge (:172-177), `save_event(spp) -> bool` (isSaveEvent, :150) and
        `regenerate_camera()` between launches (:146-148).  `save_event` may return 2 for "merge now, no extra poll"
        (scene.shouldFinalizeBuffer()); `poll_gate() -> bool` gates the timed poll only (`!manager.shouldFinalize()`, :154).
        Returns the new scene.spp."""
        assert sample_buffer.dtype == np.float64 and sample_buffer.size == self.width * self.height * 3
        spp = C.c_int32(scene_spp)
        cb = native.RunCallbacks(
            C.sizeof(native.RunCallbacks), native.POST_RENDER_FN((lambda _u: 1 if self.post_render() else 0) if self.post_render else 0),
            native.PROGRESS_FN((lambda _u, s: progress(s)) if progress else 0),
            native.PROGRESS_FN((lambda _u, s: merged(s)) if merged else 0),
            native.SAVE_EVENT_FN((lambda _u, s: int(save_event(s))) if save_event else 0),
            native.REGEN_FN((lambda _u: regenerate_camera()) if regenerate_camera else 0), None,
            native.POST_RENDER_FN((lambda _u: 1 if poll_gate() else 0) if poll_gate else 0))
        rc = native.lib().chunky_render_run_ex(self._h, ptr(sample_buffer), C.byref(spp), target_spp, merge_interval, C.byref(cb))
        if rc not in (0, native.E_ABORTED):
            check(rc)
        return spp.value

    def close(self) -> None:
        if self._h:
            check(native.lib().chunky_render_destroy(self._h))
            self._h = C.c_void_p()


def render_tiled(scene_loader: HipSceneLoader, canvas_w: int, canvas_h: int, tile_w: int, tile_h: int, seeds, projector_type: int, settings,
                 lens=None, options=None, x_cuts=None, y_cuts=None) -> np.ndarray:
    """A canvas_w x canvas_h frame rendered window by window (chunky_render_set_canvas) and assembled: bit for bit the image one
    target of the canvas's size renders from the same seeds.  The canvas is cut into a grid of tile_w x tile_h windows (the last
    column and row smaller), or, with x_cuts / y_cuts, at those columns / rows; one render target per window size is created and
    reused, reset between windows.  `lens` = (aperture, focus) for a projected camera, `options` = {option: value}.  A camera of
    pre-generated rays (type -1) is not served: its table is per window.  Returns the canvas_h x canvas_w x 3 float32 image."""
    if projector_type == native.PROJ_PREGENERATED:
        raise ValueError("render_tiled: a table of pre-generated rays is per window; crop it and call set_canvas yourself")

    def edges(total, step, cuts):
        if cuts is None:
            if step <= 0:
                raise ValueError("render_tiled: tile size must be positive")
            cuts = range(step, total, step)
        e = [0] + sorted(set(int(c) for c in cuts)) + [total]
        if any(b <= a for a, b in zip(e, e[1:])):
            raise ValueError("render_tiled: cuts must lie strictly inside the canvas")
        return e

    xs, ys = edges(canvas_w, tile_w, x_cuts), edges(canvas_h, tile_h, y_cuts)
    frame = np.zeros((canvas_h, canvas_w, 3), np.float32)
    targets = {}
    try:
        for y0, y1 in zip(ys, ys[1:]):
            for x0, x1 in zip(xs, xs[1:]):
                w, h = x1 - x0, y1 - y0
                r = targets.get((w, h))
                if r is None:
                    r = targets[(w, h)] = HipPathTracingRenderer(scene_loader, w, h)
                    for k, v in (options or {}).items():
                        r.set_option(k, v)
                    r.set_canvas(canvas_w, canvas_h, x0, y0)  # (ahead of the camera: a stacked ODS camera is checked on the canvas's height)
                    r.set_camera(projector_type, settings)
                    if lens is not None:
                        r.set_lens(*lens)
                else:
                    r.set_canvas(canvas_w, canvas_h, x0, y0)
                    r.reset()
                r.render_passes(seeds)
                frame[y0:y1, x0:x1] = r.read().reshape(h, w, 3)
    finally:
        for r in targets.values():
            r.close()
    return frame


class HipPostProcessingFilter:
    """GPU tone mapping — GpuPostProcessingFilter / ImposterCombinationGpuPostProcessingFilter
    (tonemap/GpuPostProcessingFilter.java:14-82): takes the name, description and id of the Chunky
    filter it stands in for (ChunkyCl.java:60-63: GAMMA, TONEMAP1, TONEMAP2 = ACES, TONEMAP3 = HABLE)
    and runs the `filter` kernel (tonemap/include/post_processing_filter.cl:5-51) in process_frame."""

    GAMMA, TONEMAP1, ACES, HABLE = 0, 1, 2, 3
    IMPOSTERS = {"GAMMA": GAMMA, "TONEMAP1": TONEMAP1, "TONEMAP2": ACES, "TONEMAP3": HABLE}

    def __init__(self, filter_id: str, instance: Optional[RendererInstance] = None, name: str = None, description: str = None):
        if filter_id not in self.IMPOSTERS:
            raise ValueError(f"no GPU filter for post-processing id {filter_id!r}")
        self.instance = instance or RendererInstance.get()
        self.id, self.type = filter_id, self.IMPOSTERS[filter_id]
        self.name = name or filter_id
        self.description = description or filter_id

    def get_id(self) -> str:
        return self.id

    def get_name(self) -> str:
        return self.name

    def get_description(self) -> str:
        return self.description

    def process_frame(self, width: int, height: int, input_samples: np.ndarray, output_argb: np.ndarray, exposure: float) -> None:
        """processFrame (GpuPostProcessingFilter.java:40-65): `input_samples` = width*height*3 doubles, `output_argb` =
        width*height int32 (BitmapImage.data); blocking."""
        if input_samples.dtype != np.float64 or input_samples.size != 3 * width * height or not input_samples.flags.c_contiguous:
            raise ValueError("input must be a contiguous float64 array of width*height*3 samples")
        if output_argb.dtype not in (np.int32, np.uint32) or output_argb.size != width * height or not output_argb.flags.c_contiguous:
            raise ValueError("output must be a contiguous int32 array of width*height pixels")
        check(native.lib().chunky_filter_frame(self.instance._h, width, height, float(exposure), ptr(input_samples),
                                               ptr(output_argb), self.type))

    def process_frame_alpha(self, width: int, height: int, input_samples: np.ndarray, alpha: np.ndarray, output_argb: np.ndarray,
                            exposure: float) -> None:
        """process_frame with the alpha byte of each pixel from `alpha` (width*height float32, e.g. read_aov_ex(native.AOV_ALPHA)):
        chunky_filter_frame_alpha."""
        if input_samples.dtype != np.float64 or input_samples.size != 3 * width * height or not input_samples.flags.c_contiguous:
            raise ValueError("input must be a contiguous float64 array of width*height*3 samples")
        if alpha.dtype != np.float32 or alpha.size != width * height or not alpha.flags.c_contiguous:
            raise ValueError("alpha must be a contiguous float32 array of width*height values")
        if output_argb.dtype not in (np.int32, np.uint32) or output_argb.size != width * height or not output_argb.flags.c_contiguous:
            raise ValueError("output must be a contiguous int32 array of width*height pixels")
        check(native.lib().chunky_filter_frame_alpha(self.instance._h, width, height, float(exposure), ptr(input_samples), ptr(alpha),
                                                     ptr(output_argb), self.type))

    def process_device(self, n_pixels: int, exposure: float, d_input: int, d_argb: int, repeat: int = 1) -> float:
        """The same kernel on device buffers; returns the mean kernel time in ms (HIP events)."""
        ms = C.c_float()
        check(native.lib().chunky_filter_frame_device(self.instance._h, n_pixels, float(np.float32(exposure)), C.c_void_p(d_input),
                                                      C.c_void_p(d_argb), self.type, repeat, C.byref(ms)))
        return ms.value


def adaptive_host(samples, params=None):
    """The specification of adaptive sampling on the host (native.adaptive_host): (counts, image, noise) for per-pass samples."""
    return native.adaptive_host(samples, params)


def pool_slot_order(width: int, height: int) -> np.ndarray:
    """Every pixel index of a width x height image in whole-image pool-slot order — 16 x 16 tiles row-major, 2 x 2 sub-blocks row-major
    inside a tile, row-major inside a sub-block (csrc/path_state.hpp pool_slot_gid with one rank), padding slots left out: the order of
    the active list chunky_render_adaptive builds."""
    bw, bh = (width + 15) // 16, (height + 15) // 16
    i = np.arange(256)
    sb, px = i // 4, i % 4
    dx, dy = (sb % 8) * 2 + px % 2, (sb // 8) * 2 + px // 2
    b = np.arange(bw * bh)
    x = ((b % bw) * 16)[:, None] + dx[None, :]
    y = ((b // bw) * 16)[:, None] + dy[None, :]
    keep = (x < width) & (y < height)
    return (y * width + x)[keep].astype(np.int32)
