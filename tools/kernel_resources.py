#!/usr/bin/env python3
"""tools/kernel_resources.py [out.json] — registers, spills and occupancy of every render_pool / fold_kernel instantiation, of the
denoise kernels, of the adaptive-sampling kernels, of the first-hit pass kernels (first_hit_kernel with the AOV, AOV-ex and ID-matte folds) and of the matte read-outs as hipcc reports them for gfx950
(-Rpass-analysis=kernel-resource-usage on csrc/render_pool.hip, csrc/render_pool_bvh.hip (the entity-BVH instantiations),
csrc/denoise.hip, csrc/adaptive.hip, csrc/robust.hip (fold_buckets_kernel<M>, robust_resolve_kernel<M>), csrc/aov.hip, csrc/matte.hip, csrc/occlusion.hip (occlusion_kernel), csrc/lights.hip (light_kernel, light_mix_kernel) and csrc/lights_groups.hip (light_group_kernel, light_group_mix_kernel) with the library's flags),
and of the biome-tint units csrc/render_pool_biome.hip, csrc/render_pool_biome_bvh.hip, csrc/render_biome.hip and csrc/aov_biome.hip, whose kernels are listed as "biome <name>" (they
have the names of the kernels they are instantiated from and the biome map as one more argument), and of the ground-fog units
csrc/render_pool_fog.hip and csrc/render_pool_fog_bvh.hip, listed as "fog <name>" likewise, and of the translucent-block units
csrc/render_pool_glass.hip and csrc/render_pool_glass_bvh.hip, listed as "glass <name>".  CPU only."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chunkyclplugin_amd import native  # noqa: E402

flags = [f for f in native.HIPCC_FLAGS if f not in ("-shared",)]
err = ""
for src in ("render_pool.hip", "render_pool_bvh.hip", "denoise.hip", "adaptive.hip", "robust.hip", "aov.hip", "matte.hip", "occlusion.hip", "lights.hip", "lights_groups.hip",
            "render_pool_biome.hip", "render_pool_biome_bvh.hip", "render_biome.hip", "aov_biome.hip", "render_pool_fog.hip", "render_pool_fog_bvh.hip",
            "render_pool_glass.hip", "render_pool_glass_bvh.hip"):
    cmd = ["hipcc", *flags, "-x", "hip", "-c", os.path.join(native.CSRC, src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    err += "Unit: " + src + "\n" + subprocess.run(cmd, capture_output=True, text=True).stderr
out, cur, prefix = {}, None, ""
for line in err.splitlines():
    if line.startswith("Unit: "):
        prefix = "biome " if "biome" in line else ("fog " if "_fog" in line else ("glass " if "_glass" in line else ""))
        continue
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        cur = out.setdefault(prefix + re.sub(r"\(.*", "", name).replace("chunky::", ""), {})
        continue
    for key, pat in (("sgprs", r"TotalSGPRs: (\d+)"), ("vgprs", r" VGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                     ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sgpr_spills", r"SGPRs Spill: (\d+)"), ("vgpr_spills", r"VGPRs Spill: (\d+)")):
        m = re.search(pat, line)
        if m and cur is not None:
            cur[key] = int(m.group(1))
res = {"source": "hipcc -Rpass-analysis=kernel-resource-usage, flags " + " ".join(flags), "kernels": out}
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kernel_resources.json")
json.dump(res, open(path, "w"), indent=1)
print(path, len(out), "kernels")
