"""The oracle closure above octree depth 10.  tests/golden/deep.npz holds whole 64 x 48 images of the golden scenes "outdoor",
"entities", "inside" and "pregen" at the origin of octrees of depth 11, 13, 15 and 16 (scenes.embed_deeper: the same world, a few
8-int groups in front), and of "outdoor" in a depth-12 octree at x = z = 1024 beside a full-cube leaf of level 6 — rendered by the
REFERENCE build (oracle/_ref, tests/golden/generate.py deep).  The C restatement must reproduce every one bit for bit, so that GPU
parity on the deep tree forms (tests/test_gpu_deep_trees.py: two and three 8^3 levels under the dense top, and no wide tree at all)
does not rest on the restatement being right where it has never been compared.

What the images see, measured on the reference build's own images (share of pixels that differ from the same scene rendered with
draw depth 0, i.e. without the octree; the four depths of a scene give the same image, as they must — the world is the same):
outdoor 0.637, entities 0.419, inside 1.000, pregen 0.255, outdoor at x = z = 1024 (the offset did not have to be halved) 0.652."""
import os

import numpy as np
import pytest

import golden_scenes as gs
from oracle import binding
from oracle.binding import PortOptions

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "deep.npz"))
CASES = dict(gs.embed_cases())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_file_holds_every_case():
    assert len(CASES) == 17
    assert sorted(k[:-7] for k in GOLD.files if k.endswith("_digest")) == sorted(CASES)
    assert GOLD["seeds"].tolist() == gs.scenes.java_random_ints(gs.N_PASSES).tolist()
    depths = {key: sc.octree_depth for key, sc in CASES.items()}
    assert sorted(set(depths.values())) == [11, 12, 13, 15, 16]


@pytest.mark.parametrize("key", list(CASES))
def test_restatement_matches_the_reference_in_deep_octrees(port, key):
    sc = CASES[key]
    assert gs.input_digest(sc) == str(GOLD[key + "_digest"]), "regenerated scene differs from the one the golden image was made from"
    h = binding.SceneHandle(sc)
    np.testing.assert_array_equal(bits(port.render_passes(h, GOLD["seeds"])), bits(GOLD[key + "_res"]))
    np.testing.assert_array_equal(port.preview(h), GOLD[key + "_preview"])


@pytest.mark.parametrize("key", list(CASES))
def test_the_golden_images_see_the_world(port, key):
    """Usefulness of the fixture, measured on the reference build's image: at least a quarter of its pixels (a tenth in the offset
    case, where the reference's own march loses its 1e-4 offset to the float spacing at x = 1024) differ from the image without the
    octree (draw depth 0: sky, and entities where there are any).  Shares: module docstring."""
    sc = CASES[key]
    with PortOptions(port, 0, 5, 13.0):
        sky = port.render_passes(sc, GOLD["seeds"])
    differ = (bits(GOLD[key + "_res"]).reshape(-1, 3) != bits(sky).reshape(-1, 3)).any(axis=1)
    share = float(differ.mean())
    print(f"{key}: {share:.3f} of the pixels see the octree")
    assert share >= (0.10 if key == gs.EMBED_OFFSET else 0.25), share


def test_reference_still_gives_a_committed_deep_image(ref):
    """Where the reference build exists: the depth-15 entity image and the offset image are what it returns today."""
    for key in ("entities_d15", gs.EMBED_OFFSET):
        h = binding.SceneHandle(CASES[key])
        np.testing.assert_array_equal(bits(ref.render_passes(h, GOLD["seeds"])), bits(GOLD[key + "_res"]))
        np.testing.assert_array_equal(ref.preview(h), GOLD[key + "_preview"])
