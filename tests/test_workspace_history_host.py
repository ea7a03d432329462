"""CPU suite: the inputs of the workspace-history tests are what tests/history_inputs.py claims, measured on the oracle's stage
arrays -- so the GPU test cannot pass because a predecessor quietly became small or tame.  No GPU call is made here."""
import functools
import hashlib

import numpy as np
import pytest

import chain_inputs as ci
import history_inputs as hi

BLOCK = 4096                                                   # records per block of a context chain (kernels_e1.hip)


@functools.lru_cache(maxsize=None)
def _measure(key):
    """(pixels, bins, largest symbol, most bins of a pixel, contexts used, longest context chain) of one plane."""
    from oracle.oracle import Oracle
    st = Oracle().stages(_PLANES[key])
    chains = np.bincount(st["adr"].astype(np.int64), minlength=2048)
    return dict(px=int(st["z"].size), bins=int(st["cu"].size), z_max=int(st["z"].max()), cnt_max=int(st["ev_count"].max()),
                contexts=chains > 0, chain_max=int(chains.max()))


_PLANES = {}


def measure(plane):
    key = (plane.shape, hashlib.sha256(plane.tobytes()).digest())
    _PLANES.setdefault(key, plane)
    return _measure(key)


@pytest.fixture(scope="module")
def subjects():
    """The largest of every measure over the subjects: the image subjects, and the caller-made records by their counts."""
    m = [measure(i) for _, i in hi.subject_images()] + [measure(hi.band_plane())]
    records = max(int(ci.model_families(model)[name]["x"].size) for model, name in hi.MODEL_FAMILIES)
    events = max(int(ci.back_families()[name].size) for name in hi.BACK_FAMILIES)
    return dict(px=max(max(x["px"] for x in m), records), bins=max(max(x["bins"] for x in m), events),
                cnt_max=max(x["cnt_max"] for x in m), density=max(x["bins"] / x["px"] for x in m if x["px"] >= 100))     # (a 1 x 1 image's first pixel is no density)


def test_hostile_planes_reach_the_extremes(subjects):
    m = [measure(p) for p in hi.hostile_planes()]
    assert max(x["z_max"] for x in m) == 255                                   # a symbol of 255
    assert min(x["cnt_max"] for x in m) > subjects["cnt_max"]                  # every hostile plane: a pixel with more bins than any subject's
    assert min(x["bins"] / x["px"] for x in m) > subjects["density"]           # and more bins per pixel on average
    used = np.bincount(hi.hostile_records()[2].astype(np.int64), minlength=2048) > 0      # the records behind the batch
    for x in [measure(p) for p in hi.hostile_e1_planes()]:
        used |= x["contexts"]
    assert used.all()                                                          # every one of the 2048 contexts
    small = [measure(c[0]) for c in hi.serial_cases()[:3]]
    assert max(x["z_max"] for x in small) == 255 and min(x["cnt_max"] for x in small) > subjects["cnt_max"]


def test_flat_planes_have_chains_of_many_blocks():
    m = [measure(p) for p in hi.flat_planes()]
    assert all(x["chain_max"] > 2 * BLOCK for x in m)                          # a chain longer than two blocks in every plane
    assert max(x["chain_max"] for x in m) > 20 * BLOCK


@pytest.mark.parametrize("name", [p for p in hi.PREDECESSORS if p != "fresh"])
def test_every_predecessor_dwarfs_the_subjects(subjects, name):
    m = [measure(p) for p in hi.predecessor_planes(name)]
    assert sum(x["px"] for x in m) >= 4 * subjects["px"], name
    assert sum(x["bins"] for x in m) >= 4 * subjects["bins"], name
    # and in every slot a predecessor's first launch fills: the slot's plane alone is larger than any subject
    first = m[:hi.BATCH]
    assert min(x["px"] for x in first) >= subjects["px"] and min(x["bins"] for x in first) >= subjects["bins"], name
    assert first[0]["px"] == max(x["px"] for x in m)                           # slot 0, where the debug hooks run: the largest


def test_subject_calls_are_one_launch_each():
    assert all(len(b) <= hi.BATCH for b in hi.subject_batches()) and len(hi.rotation_batch()) == hi.BATCH == len(hi.small_pack())
    assert sum(len(b) for b in hi.subject_batches()) == len(hi.SHAPES) * len(hi.CONTENTS)
    assert sorted(p.size for p in hi.small_pack())[0] == 1 and max(p.size for p in hi.small_pack()) == 300
