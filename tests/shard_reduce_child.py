"""Child process of tests/test_gpu_shard_map.py: a group on the reduce transport renders the outdoor golden scene at the views
and outer shares the parent lists, each into a caller's buffer full of a marker, and saves what read() returns.  A process of its
own because the RCCL binding is made once per process (csrc/rccl_dyn.hpp) and the rig variables are read at group creation.

    shard_reduce_child.py <devices, e.g. 0,0,0> <cells as JSON: [[width, height, rank, world, tile], ...]> <marker> <output .npz>"""
import json
import os
import sys

import numpy as np
import torch  # before the library loads: torch brings a HIP runtime of its own, and the second runtime of a process finds no device

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import golden_scenes as gs  # noqa: E402
from chunkyclplugin_amd import native  # noqa: E402
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance  # noqa: E402


def main():
    devices = [int(d) for d in sys.argv[1].split(",")]
    cells, marker, path = json.loads(sys.argv[2]), float(sys.argv[3]), sys.argv[4]
    seeds = native.java_random_ints(2)
    base = gs.make("outdoor")
    inst = RendererInstance.group(devices)
    info = {"members": inst.group_size(), "before": inst.transport(), "during": []}
    loader = HipSceneLoader(inst)
    loader.load_packed(base)
    targets, images = {}, {}
    for w, h, rank, world, tile in cells:
        if (w, h) not in targets:
            sc = base.with_view(w, h)
            targets[w, h] = HipPathTracingRenderer(loader, w, h)
            targets[w, h].set_camera(sc.projector_type, sc.camera)
        r = targets[w, h]
        fb = torch.full((3 * w * h,), marker, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.set_device_buffer(fb.data_ptr())
        try:
            r.set_shard(rank, world, tile)
            r.render_passes(seeds)
            images[f"{w}x{h}:{rank},{world},{tile}"] = r.read()
        finally:
            r.set_device_buffer(None)
        info["during"].append(inst.transport()["name"])
    info["after"] = inst.transport()
    for r in targets.values():
        r.close()
    loader.close()
    inst.close()
    np.savez(path, info=json.dumps(info), **images)
    print(json.dumps(info), flush=True)


if __name__ == "__main__":
    main()
