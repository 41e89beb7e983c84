"""Every index array and layout of ``pocomc_amd/maf_spec.py`` against what the parent commit's code built
(``tests/golden/maf_spec_images_parent.json``: dtype, shape and sha256 of every array; the layouts as they are).

The device images are gather maps into the canonical parameter vector, and the kernels read them by offsets written out on
their side, so an image is right exactly when it is byte for byte the one the kernels were built against.  The golden file
is written by the parent commit's code:

    python tests/test_maf_spec_images_cpu.py PATH/TO/PARENT/maf_spec.py COMMIT

with ``maf_spec.py`` taken from a checkout of the parent (the arrangement of ``tests/golden/inverse_queries_parent.json``).
The specs are the smallest that reach every branch of the builders."""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maf_spec_images_parent.json")

#        id                  positional arguments      keyword arguments
SPECS = {
    "d2":              ((2, 3), {}),                                      # one degree, tri_ok false, no chain-image special cases
    "d5":              ((5, 3), {}),                                      # fewer ranks than a tile, padding groups
    "d6":              ((6, 3), {}),
    "d7_h41":          ((7, 3, 41), {}),                                  # odd width, padding inside tiles
    "d16_t6":          ((16, 6), {}),                                     # six transforms, both orders
    "d32":             ((32, 3), {}),                                     # the headline shape
    "d66":             ((66, 3), {}),                                     # nOT > 8, n_dim > 64
    "d100":            ((100, 3), {}),                                    # a wide default flow, H = 512, nXT = 7
    "d16_rqs4":        ((16, 3), dict(univariate="rqs", bins=4)),
    "d32_rqs8":        ((32, 3), dict(univariate="rqs", bins=8)),
    "d8_rqs16":        ((8, 3), dict(univariate="rqs", bins=16)),
    "d32_h512_rqs8":   ((32, 3, 512, "rqs", 8), {}),
}

# first 8 hex digits of sha256 over the returned int32 arrays' bytes, concatenated in return order, measured at 5203d2b
# independently of this module: what the golden file must say too
MEASURED_AT_PARENT = {
    "d32":           dict(pack_index="87f25492", pack_index_bf16="615ae0d7", wide_index="4e630f1d", train_index="85034e80"),
    "d2":            dict(pack_index="a69ad8a1", pack_index_bf16="3687a8ab", wide_index="47e6f166", train_index="b40f9e3a"),
    "d100":          dict(pack_index="e7c46b0c", pack_index_bf16="74cb95d8", wide_index="1ec7f286", train_index="ede8df9c"),
    "d32_h512_rqs8": dict(pack_index="332a6b60", pack_index_bf16="e2212920", wide_index="73372d93", train_index="e6f90e68"),
}


def _ordered(v):
    """A layout dict as nested ``[key, value]`` lists, so that the order of the keys is compared too."""
    if isinstance(v, dict):
        return [[str(k), _ordered(x)] for k, x in v.items()]
    return int(v)


def _arrays(name, ret):
    """Record of what one builder returned (an array or a tuple of arrays)."""
    ret = ret if isinstance(ret, tuple) else (ret,)
    assert all(isinstance(a, np.ndarray) for a in ret), name
    whole = hashlib.sha256()
    for a in ret:
        whole.update(np.ascontiguousarray(a).tobytes())
    return dict(arrays=[dict(dtype=str(a.dtype), shape=list(a.shape),
                             sha256=hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()) for a in ret],
                sha256_concatenated=whole.hexdigest())


def collect(MAFSpec, key):
    args, kw = SPECS[key]
    s = MAFSpec(*args, **kw)
    out = {b: _arrays(b, getattr(s, b)()) for b in ("pack_index", "pack_index_bf16", "wide_index", "train_index",
                                                     "train_jobs", "train_tables", "device_meta", "mask_flat")}
    out["pk_offsets"] = _ordered(s.pk_offsets)
    out["pk_per_transform"] = int(s.pk_per_transform)
    for lay in ("bf16_layout", "wide_layout", "train_layout"):
        out[lay] = _ordered(getattr(s, lay)())
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_names_its_commit_and_covers_the_specs(golden):
    assert golden["written_by_commit"].startswith("5203d2b")
    assert list(golden["specs"]) == list(SPECS)
    for key, want in MEASURED_AT_PARENT.items():
        for builder, h8 in want.items():
            rec = golden["specs"][key][builder]
            assert rec["sha256_concatenated"][:8] == h8, (key, builder)
            assert all(a["dtype"] == "int32" for a in rec["arrays"]), (key, builder)


@pytest.mark.parametrize("key", list(SPECS))
def test_every_image_and_layout_is_the_parents(golden, key):
    from pocomc_amd.maf_spec import MAFSpec
    got, want = collect(MAFSpec, key), golden["specs"][key]
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], (key, name)


def record(maf_spec_py, commit):
    mod_spec = importlib.util.spec_from_file_location("maf_spec_parent", maf_spec_py)
    mod = importlib.util.module_from_spec(mod_spec)
    sys.modules[mod_spec.name] = mod                        # (dataclasses looks the module up while the class is built)
    mod_spec.loader.exec_module(mod)
    out = dict(written_by_commit=commit,
               what="dtype, shape and sha256 of every index array of MAFSpec, and its layouts, as the named commit's "
                    "pocomc_amd/maf_spec.py builds them (tests/test_maf_spec_images_cpu.py)",
               specs={key: collect(mod.MAFSpec, key) for key in SPECS})
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return GOLDEN


if __name__ == "__main__":
    print(record(sys.argv[1], sys.argv[2]))
