"""Shared helpers for the parity tests (test infrastructure; may import the oracle)."""
import contextlib
import os

import numpy as np
import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def val_module():
    """The repository's test.py as a module (`import test` would find the standard library's): a fresh one per call, so the names a test
    replaces on it stay with that test."""
    import importlib.util
    import sys
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    spec = importlib.util.spec_from_file_location("icaf_root_test", os.path.join(REPO, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sample_idx(numel, tag, n=2048):
    """Same seeded sampling as tests/golden/make_golden.py."""
    g = np.random.default_rng([0x5A3917, tag])
    return g.integers(0, numel, size=min(n, numel))


def load_cfg(yaml_name):
    with open(os.path.join(REPO, "models", "transformer", yaml_name)) as f:
        return yaml.safe_load(f)


def state_dict_shapes_from_oracle_cfg(cfg):
    """Build the reference-compatible state_dict layout from our own (CPU-constructible) Model."""
    from icafusion_amd.models.yolo import Model
    return Model(cfg)


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def rel_err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def golden_logits(g, logits):
    """(ours, the golden's) class logits of a model fixture: the whole tensor, or — for a fixture that recorded only seeded samples
    of them (`logits_shape`, make_golden.py `sample_logits`) — ours sampled at the same indices."""
    logits = np.asarray(logits)
    if "logits_shape" not in g.files:
        return logits, g["logits"]
    assert tuple(logits.shape) == tuple(g["logits_shape"]), (logits.shape, g["logits_shape"])
    return logits.reshape(-1)[sample_idx(logits.size, 99)], g["logits"]


@contextlib.contextmanager
def lib_option(name, value):
    """Set one of libicaf.so's probe knobs (options.PlanOptions fields tagged lib=True) for the body of a `with`, and restore the
    process's own value afterwards.  The knobs are pushed into the library once, when it is loaded: writing ICAF_OPTIONS or a legacy
    variable into os.environ later changes nothing (tests/test_host_logic.py guards against such writes)."""
    from icafusion_amd import _lib
    from icafusion_amd.options import OPT
    restore = OPT.lib_options()[name]
    lib = _lib.lib()
    _lib.check(lib.icaf_set_option(name.encode(), int(value)), f"icaf_set_option({name}, {value})")
    try:
        yield
    finally:
        _lib.check(lib.icaf_set_option(name.encode(), int(restore)), f"icaf_set_option({name}, {restore})")
