"""
The models' host layer without a GPU: the packed-weight cache of ModelBase driven with CPU tensors and a counting pack
callable, and the Dense-stack layout of learn_nerf.params (spec rows, views, initialisation) behind the four models.
The sha256 values were recorded before the three per-model copies of that layout were replaced by the shared functions:
they pin the spec and, through init_flat_ with seed 0, the order in which the generator is consumed.
"""
import gc
import hashlib
import weakref

import pytest
import torch

from learn_nerf.instant_ngp import InstantNGPModel, InstantNGPRefNERFModel
from learn_nerf.model import ModelBase, NeRFModel
from learn_nerf.params import as_generator, build_tree, dense_views
from learn_nerf.ref_nerf import RefNERFModel


class CountingPack:
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return torch.full((4,), self.calls, dtype=torch.uint8)


def test_pack_cache_hits_and_misses():
    model, pack = ModelBase(), CountingPack()
    flat = torch.zeros(8)
    first = model._packed("bf16", flat, 4, pack)
    assert model._packed("bf16", flat, 4, pack) is first and pack.calls == 1
    split = model._packed("split", flat, 4, pack)  # the kinds do not share an entry
    assert split is not first and pack.calls == 2
    assert model._packed("split", flat, 4, pack) is split and model._packed("bf16", flat, 4, pack) is first
    flat.add_(1.0)  # an in-place op bumps the version counter
    second = model._packed("bf16", flat, 4, pack)
    assert pack.calls == 3 and second is not first
    model.invalidate_packed()  # writes that torch does not see
    third = model._packed("bf16", flat, 4, pack)
    assert pack.calls == 4 and third is not second
    # every miss returned a new buffer and left the earlier ones as they were
    assert [int(t[0]) for t in (first, split, second, third)] == [1, 2, 3, 4]
    model._pack_cache = None  # how tests empty the cache from outside
    assert model._packed("bf16", flat, 4, pack) is not third and pack.calls == 5
    other = ModelBase()  # the counters are per instance
    assert other._pack_cache is None and other._pack_generation == 0 and model._pack_generation == 1


def test_pack_cache_entry_keeps_its_source_tensor_alive():
    model, pack = ModelBase(), CountingPack()
    flat = torch.zeros(8)
    ref = weakref.ref(flat)
    model._packed("bf16", flat, 4, pack)
    del flat
    gc.collect()
    assert ref() is not None  # so a freed temporary's address cannot come back as a stale hit
    model._pack_cache = None
    gc.collect()
    assert ref() is None


def test_pack_cache_evicts_the_least_recently_used_entry():
    model, pack = ModelBase(), CountingPack()
    a, b, c = torch.zeros(8), torch.zeros(8), torch.zeros(8)
    pa = model._packed("bf16", a, 2, pack)
    model._packed("bf16", b, 2, pack)
    assert model._packed("bf16", a, 2, pack) is pa  # a hit refreshes recency: b is now the oldest
    model._packed("bf16", c, 2, pack)  # capacity + 1
    assert len(model._pack_cache) == 2 and pack.calls == 3
    assert model._packed("bf16", a, 2, pack) is pa and pack.calls == 3
    model._packed("bf16", b, 2, pack)
    assert pack.calls == 4  # b was evicted


NGP = dict(table_sizes=[2 ** 8] * 3, grid_sizes=[4, 8, 16], bbox_min=(-1.0,) * 3, bbox_max=(1.0,) * 3)  # dense + 2 hashed
LAYOUTS = {
    "nerf": (lambda: NeRFModel(), 593924,
             "7a1e4cdd0009f380ebd05f8c5ce88662b13574147481ecdde53954872f5a3878",
             "8fc806d6ea9511ffd3328a8995b1f42dd916e9523cce1a2ad138d39e33ba90af"),
    "refnerf": (lambda: RefNERFModel(), 592771,
                "29930a8f14ef56ef59ad6da011b6e63da81a49e1ac0b7f99da03423d367daed1",
                "71802643360910396b8d96d01b9ddb705c4a5d089b2c34d71359b357bd0c0629"),
    "ngp": (lambda: InstantNGPModel(**NGP), 9619,
            "b39f4c3c10049c7237fa544942dcb1f14ef530324f3587da4f345676c2c36e85",
            "c6dbe9de2289ee06e3a054c0c63f2b5d1595c99d6f36f95e222951aa05d7bd2d"),
    "ngpref": (lambda: InstantNGPRefNERFModel(**NGP), 9171,
               "ff12a587bb3787b33356765f2c1d1825ddf3f89b3fb4296f4c2826dd2bfc17ff",
               "68e8ddf111b3e0b25d1c125c325d85e36af26481d2c27a957a4fde3e4e8d90c9"),
    "nerf_1_1": (lambda: NeRFModel(input_layers=1, mid_layers=1), 133380,
                 "ab3aa0bd7ac89f5646dbecd9a1e97db742233e8e124c2340be4a289a01992fd6",
                 "258be792e1d46f9524ff8292e1d351dae1a2a96aa4c983ad8aac7c22e49f62e5"),
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_param_spec_and_init_are_unchanged(name):
    make, count, spec_sha, init_sha = LAYOUTS[name]
    model = make()
    assert model.num_params() == count
    assert hashlib.sha256(repr(model.param_spec()).encode()).hexdigest() == spec_sha
    flat = torch.zeros(count, dtype=torch.float32)
    model.init_flat_(flat, as_generator(0))
    assert hashlib.sha256(flat.numpy().tobytes()).hexdigest() == init_sha


@pytest.mark.parametrize("name", ["nerf_1_1", "ngp"])
def test_dense_views_alias_the_flat_buffer_where_build_tree_does(name):
    model = LAYOUTS[name][0]()
    flat = torch.zeros(model.num_params())
    tree = build_tree(flat, model.param_spec())
    if name == "ngp":  # the hash tables precede the Dense block
        dims, off = model.dense_dims(), model.encoding().num_table_floats()
        assert off == 2 * (4 ** 3 + 2 ** 8 + 2 ** 8)
    else:
        dims, off = model.layer_dims(), 0
    views = dense_views(flat, dims, off)
    assert len(views) == len(dims)
    for i, (kernel, bias) in enumerate(views):
        for view, leaf in ((kernel, tree[f"Dense_{i}"]["kernel"]), (bias, tree[f"Dense_{i}"]["bias"])):
            assert view.shape == leaf.shape and view.data_ptr() == leaf.data_ptr() and view.stride() == leaf.stride()
        bias.fill_(float(i + 1))  # a view, not a copy
        assert float(tree[f"Dense_{i}"]["bias"][0]) == i + 1
    assert int((flat != 0).sum()) == sum(fo for _, fo in dims)
