"""Regenerates tests/golden/*.npz by running the REFERENCE kernel (oracle/_ref: rayTracer.cl compiled
in place from /root/reference for x86-64).  Only works in the build container.

    python tests/golden/generate.py

Each file holds, for one named scene of tests/golden_scenes.py: the sha256 of the regenerated
inputs, the `res` buffer after N_PASSES passes with the java.util.Random(0) seed stream, the
`preview` ARGB image, and per-trace hit records + radiance for RECORD_GIDS at seed[0].
kats.npz holds the function-level known answers (PCG stream, seed stream, sun basis, builtins).
filter.npz (`python tests/golden/generate.py filter` writes only this one) holds the reference tone-map
kernel (tonemap/include/post_processing_filter.cl, compiled in place the same way): sample values,
exposures, and the ARGB words for every filter type, plus pow known answers.
timed_rows.npz (`... generate.py timed`): rows of the five BASELINE views at their timed sizes (write_timed).
timed_camera_rows.npz (`... generate.py cameras`): rows of the camera / tint / atlas views at the timed sizes (write_cameras).
helpers.npz (`... generate.py helpers`): known answers of the reference's exported helper functions (write_helpers).
deep.npz (`... generate.py deep`): the golden worlds inside octrees of depth 11 - 16 (write_deep).
timed_big_rows.npz (`... generate.py timed` writes it beside timed_rows.npz): eight rows of the beyond-cache view (write_timed_big).
routes.npz (`... generate.py routes`): the exhibits of tests/route_scenes.py — the routes no other fixture reaches (write_routes).
libm_platform.npz (`... generate.py libm`): images of the reference object on a second platform layer (glibc libm): write_libm.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import golden_scenes as gs  # noqa: E402
from chunkyclplugin_amd import scenes  # noqa: E402
from oracle import binding  # noqa: E402


FILTER_EXPOSURES = (1.0, 0.37, 1.5)
FILTER_TYPES = (0, 1, 2, 3, 7)


def filter_samples():
    """Sample-buffer values inside the domain where the reference's float -> uint conversion is defined."""
    rng = np.random.default_rng(2024)
    x = np.concatenate([rng.uniform(0, 2, 3000), 10.0 ** rng.uniform(-45, 6, 2400), rng.uniform(0, 0.02, 594),
                        [0.0, 0.004, 1.0, 1e-310, 5e-324, 1e6]])
    rng.shuffle(x)
    return x


def write_filter(ref):
    x = filter_samples()
    out = np.stack([np.stack([ref.filter(x, e, t) for e in FILTER_EXPOSURES]) for t in FILTER_TYPES])
    rng = np.random.default_rng(7)
    pa = np.concatenate([rng.uniform(0, 4, 3000), 10.0 ** rng.uniform(-44, 8, 1000)]).astype(np.float32)
    pb = np.concatenate([rng.uniform(-3, 3, 2000), np.full(2000, 1.0 / 2.2)]).astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "filter.npz"), samples=x, exposures=np.array(FILTER_EXPOSURES),
                        types=np.array(FILTER_TYPES), argb=out, pow_a=pa, pow_b=pb, pow=ref.pow(pa, pb))
    print("filter written", out.shape)


def write_timed(ref):
    """timed_rows.npz: whole image rows of the BASELINE views AT THE SIZES THAT ARE TIMED (golden_scenes.timed_view), rendered
    by the reference build — TIMED_PASSES passes of the java.util.Random(0) seed stream — so that parity at depth-9/10 octrees
    and height-17 BVHs does not rest on the C restatement."""
    seeds = scenes.java_random_ints(gs.TIMED_PASSES)
    out = {"seeds": seeds}
    for name in gs.TIMED_VIEWS:
        sc = gs.timed_view(name)
        h = binding.SceneHandle(sc)
        rows = gs.timed_rows(sc)
        res = np.zeros((len(rows), sc.width, 3), np.float32)
        for k, y in enumerate(rows):
            full = ref.render_passes(h, seeds, gid_range=(y * sc.width, (y + 1) * sc.width), threads=8)
            res[k] = full.reshape(-1, 3)[y * sc.width:(y + 1) * sc.width]
        out[name + "_digest"] = gs.input_digest(sc)
        out[name + "_rows"] = np.array(rows, np.int32)
        out[name + "_res"] = res
        print(name, sc.width, sc.height, "rows", rows, "mean", float(res.mean()), flush=True)
    np.savez_compressed(os.path.join(HERE, "timed_rows.npz"), **out)


def write_timed_big(ref):
    """timed_big_rows.npz: eight whole rows (golden_scenes.camera_rows) of the view bench.py --config 5 times — the 128 x 128-chunk
    world, a depth-11 octree: a dense top over TWO 8^3 levels — rendered by the reference build, TIMED_PASSES passes of the
    java.util.Random(0) seed stream."""
    seeds = scenes.java_random_ints(gs.TIMED_PASSES)
    sc = gs.timed_view("big")
    h = binding.SceneHandle(sc)
    rows = gs.camera_rows(sc)
    res = np.zeros((len(rows), sc.width, 3), np.float32)
    for k, y in enumerate(rows):
        full = ref.render_passes(h, seeds, gid_range=(y * sc.width, (y + 1) * sc.width), threads=binding.usable_threads())
        res[k] = full.reshape(-1, 3)[y * sc.width:(y + 1) * sc.width]
    print("big", sc.width, sc.height, "rows", rows, "mean", float(res.mean()), flush=True)
    savez_lzma(os.path.join(HERE, "timed_big_rows.npz"), seeds=seeds, big_digest=gs.input_digest(sc), big_rows=np.array(rows, np.int32), big_res=res)


def write_deep(ref):
    """deep.npz: golden_scenes.embed_cases — four golden worlds at the origin of octrees of depth 11, 13, 15 and 16, and "outdoor" in
    a depth-12 octree at x = z = 1024 beside a full-cube leaf of level 6 — whole images after the N_PASSES golden seeds, previews
    and input digests, by the reference build."""
    seeds = scenes.java_random_ints(gs.N_PASSES)
    out = {"seeds": seeds}
    for key, sc in gs.embed_cases():
        h = binding.SceneHandle(sc)
        out[key + "_digest"] = gs.input_digest(sc)
        out[key + "_res"] = ref.render_passes(h, seeds)
        out[key + "_preview"] = ref.preview(h)
        print(key, "depth", sc.octree_depth, "res mean", float(np.nanmean(out[key + "_res"])), flush=True)
    savez_lzma(os.path.join(HERE, "deep.npz"), **out)


def write_cameras(ref):
    """timed_camera_rows.npz: the same as timed_rows.npz for golden_scenes.CAMERA_VIEWS — depth of field, pre-generated rays (a
    ragged 1917 x 1075 view among them), a camera outside the world, a flooded world (whose water, tint type 3, 4 of the rows' 400 726 traces
    reach: the tint's fixture is routes.npz), textures over four atlas layers, sun
    draws in the room, the city with depth of field, and pre-generated rays into the entity world — eight rows each
    (golden_scenes.camera_rows), TIMED_PASSES passes of the java.util.Random(0) seed stream."""
    seeds = scenes.java_random_ints(gs.TIMED_PASSES)
    out = {"seeds": seeds}
    for name in gs.CAMERA_VIEWS:
        sc = gs.camera_view(name)
        h = binding.SceneHandle(sc)
        rows = gs.camera_rows(sc)
        res = np.zeros((len(rows), sc.width, 3), np.float32)
        for k, y in enumerate(rows):
            full = ref.render_passes(h, seeds, gid_range=(y * sc.width, (y + 1) * sc.width), threads=binding.usable_threads())
            res[k] = full.reshape(-1, 3)[y * sc.width:(y + 1) * sc.width]
        out[name + "_digest"] = gs.input_digest(sc)
        out[name + "_rows"] = np.array(rows, np.int32)
        out[name + "_res"] = res
        print(name, sc.width, sc.height, "rows", rows, "mean", float(res.mean()), flush=True)
    savez_lzma(os.path.join(HERE, "timed_camera_rows.npz"), **out)


def savez_lzma(path, **arrays):
    """np.savez_compressed with LZMA instead of deflate (np.load reads either): radiance rows compress about 9 % better, which
    keeps eight rows of eight 1080p views under the 1 MiB a committed file may take."""
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in arrays.items():
            with z.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def write_helpers(ref):
    """helpers.npz: answers of the reference object's own exported helpers (oracle/ref_shim.cpp ref_helpers drives them) on the
    input rows of golden_scenes.helper_rows, for the golden scene "entities" (models, textures, sun disc, both BVHs)."""
    sc = gs.make(gs.HELPER_SCENE)
    out = {"digest": gs.input_digest(sc)}
    for which in gs.HELPER_KINDS:
        rows = gs.helper_rows(sc, which)
        out[f"in{which}_sha256"] = gs.rows_digest(rows)   # the rows are regenerated from their seeds by the tests
        out[f"out{which}"] = ref.helpers(sc, which, rows)
        ok = out[f"out{which}"]
        print("helper", which, rows.shape, "finite first column:", float(np.isfinite(ok[:, 0]).mean()), flush=True)
    np.savez_compressed(os.path.join(HERE, "helpers.npz"), **out)


def write_routes(ref):
    """routes.npz: the scenes of tests/route_scenes.py (the exhibits at depth 6, embedded at depths 7, 11 and 16, and the four
    entity variants), outputs of the reference build only: the radiance after route_scenes.N_PASSES passes of the java.util.Random(0)
    seed stream, the preview, the trace records of seed[0] at every 7th pixel (the valid records of all pixels one after the other,
    for the scenes of RECORD_SCENES), the reference's own helpers 4 and 12 on rows drawn from the exhibits' palettes, input digests."""
    import route_scenes as rs
    seeds = scenes.java_random_ints(rs.N_PASSES)
    out = {"seeds": seeds}
    for name in rs.NAMES:
        sc = rs.make(name)
        h = binding.SceneHandle(sc)
        out[name + "_digest"] = gs.input_digest(sc)
        out[name + "_res"] = ref.render_passes(h, seeds)
        out[name + "_preview"] = ref.preview(h)
        if name in rs.RECORD_SCENES:
            recs, cnt, rad = [], [], []
            for g in rs.RECORD_GIDS:
                r, c = ref.trace_records(h, int(seeds[0]), int(g))
                recs.append(r.copy())
                cnt.append(len(r))
                rad.append(c.copy())
            out[name + "_records"] = np.concatenate(recs)
            out[name + "_counts"] = np.array(cnt, np.int32)
            out[name + "_radiance"] = np.array(rad, np.float32)
        print(name, "res mean", float(np.nanmean(out[name + "_res"])), flush=True)
    base = rs.make("routes")
    for which in rs.HELPER_KINDS:
        rows = rs.helper_rows(which)
        out[f"in{which}_sha256"] = gs.rows_digest(rows)
        out[f"out{which}"] = ref.helpers(base, which, rows)
    path = os.path.join(HERE, "routes.npz")
    savez_lzma(path, **out)
    print("routes written", os.path.getsize(path), "bytes")


LIBM_SPP = 32


def write_libm():
    """libm_platform.npz: the SAME reference object linked against a SECOND conforming platform layer — glibc libm and unfused
    dot / cross / normalize instead of rt_math.h (`make -C oracle ref_libm`) — renders three golden scenes at LIBM_SPP passes.
    Two conforming platforms differ in last bits, so these images are compared statistically (tests/test_platform_layer.py):
    a guard that does not share rt_math.h with what it checks.  The same file is the fixture of the BIT-EXACT pin of the
    restatement's logic: oracle/port.c built with -DPORT_LIBM (the same second platform layer) must reproduce every image, preview
    and timed row in it (all ten golden scenes, and the BASELINE views at the sizes that are timed: `timed_<view>_res`)."""
    import subprocess
    subprocess.run(["make", "-C", os.path.join(os.path.dirname(HERE), "..", "oracle"), "ref_libm"], check=True, stdout=subprocess.DEVNULL)
    libm = binding.RefLib(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "libchunky_ref_libm.so"))
    seeds = scenes.java_random_ints(LIBM_SPP)
    out = {"seeds": seeds}
    for name in gs.NAMES:
        sc = gs.make(name)
        out[name + "_digest"] = gs.input_digest(sc)
        out[name + "_res"] = libm.render_passes(binding.SceneHandle(sc), seeds)
        out[name + "_preview"] = libm.preview(binding.SceneHandle(sc))
        print("libm", name, float(out[name + "_res"].mean()), flush=True)
    tseeds = scenes.java_random_ints(gs.TIMED_PASSES)
    for name in gs.TIMED_VIEWS:
        sc = gs.timed_view(name)
        h = binding.SceneHandle(sc)
        rows = gs.timed_rows(sc)
        res = np.zeros((len(rows), sc.width, 3), np.float32)
        for k, y in enumerate(rows):
            full = libm.render_passes(h, tseeds, gid_range=(y * sc.width, (y + 1) * sc.width), threads=8)
            res[k] = full.reshape(-1, 3)[y * sc.width:(y + 1) * sc.width]
        out["timed_" + name + "_digest"] = gs.input_digest(sc)
        out["timed_" + name + "_res"] = res
        print("libm timed", name, float(res.mean()), flush=True)
    np.savez_compressed(os.path.join(HERE, "libm_platform.npz"), **out)


def main():
    ref = binding.ref()
    assert ref is not None, "needs /root/reference"
    if "filter" in sys.argv[1:]:
        return write_filter(ref)
    if "timed_big" in sys.argv[1:]:   # the new rows alone (timed_rows.npz stays as it is)
        return write_timed_big(ref)
    if "timed" in sys.argv[1:]:
        write_timed(ref)
        return write_timed_big(ref)
    if "deep" in sys.argv[1:]:
        return write_deep(ref)
    if "helpers" in sys.argv[1:]:
        return write_helpers(ref)
    if "cameras" in sys.argv[1:]:
        return write_cameras(ref)
    if "libm" in sys.argv[1:]:
        return write_libm()
    if "routes" in sys.argv[1:]:
        return write_routes(ref)
    seeds = scenes.java_random_ints(gs.N_PASSES)
    for name in gs.NAMES:
        sc = gs.make(name)
        h = binding.SceneHandle(sc)
        res = ref.render_passes(h, seeds)
        prev = ref.preview(h)
        recs = np.zeros((len(gs.RECORD_GIDS), binding.MAX_TRACES), binding.HIT_DTYPE)
        cnt = np.zeros(len(gs.RECORD_GIDS), np.int32)
        rad = np.zeros((len(gs.RECORD_GIDS), 3), np.float32)
        for i, g in enumerate(gs.RECORD_GIDS):
            r, c = ref.trace_records(h, int(seeds[0]), int(g))
            recs[i, :len(r)] = r
            cnt[i] = len(r)
            rad[i] = c
        np.savez_compressed(os.path.join(HERE, name + ".npz"), digest=gs.input_digest(sc), seeds=seeds, res=res,
                            preview=prev, records=recs, counts=cnt, radiance=rad)
        print(name, "res mean", float(np.nanmean(res)), "traces", int(cnt.sum()))
    # function-level known answers
    st, fl = ref.pcg_stream(0, 16)
    st2, fl2 = ref.pcg_stream(0xDEADBEEF, 16)
    xs = np.linspace(-7, 7, 4001).astype(np.float32)
    us = np.linspace(-1.2, 1.2, 4001).astype(np.float32)
    rng = np.random.default_rng(1)
    ya, xa = rng.normal(size=4000).astype(np.float32), rng.normal(size=4000).astype(np.float32)
    sun = scenes.pack_sun(0.174533, 1.256637, 1.25, True)
    np.savez_compressed(
        os.path.join(HERE, "kats.npz"), pcg_states0=st, pcg_floats0=fl, pcg_states1=st2, pcg_floats1=fl2,
        java_seeds=scenes.java_random_ints(8), xs=xs, us=us, ya=ya, xa=xa,
        sin=ref.math(0, xs), cos=ref.math(1, xs), asin=ref.math(2, us), acos=ref.math(3, us),
        atan2=ref.math(4, ya, xa), fmod1=ref.math(5, xs), sun=sun, sun_basis=ref.sun_basis(sun))
    print("kats written")
    write_filter(ref)
    write_timed(ref)
    write_timed_big(ref)
    write_deep(ref)
    write_cameras(ref)
    write_helpers(ref)
    write_routes(ref)
    write_libm()


if __name__ == "__main__":
    main()
