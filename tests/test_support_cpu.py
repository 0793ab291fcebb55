"""The tests' own support layer: `guarded.Guarded` on CPU tensors, and the rule that keeps the layer in one place -- no test module
imports another, `Guarded` is defined once, and the `dev` fixture is defined once (tests/support.py)."""
import ast
import glob
import os

import pytest
import torch

import backward_cases
import forward_head_cases
import layernorm_cases
import reduction_cases
from guarded import Guarded

SLACK = reduction_cases.SLACK
TESTS = os.path.dirname(os.path.abspath(__file__))


def test_every_case_module_keeps_64_floats_behind_a_buffer():
    assert SLACK == backward_cases.SLACK == forward_head_cases.SLACK == layernorm_cases.SLACK == 64


@pytest.mark.parametrize("off", [0, 1, SLACK])
def test_guarded_on_cpu_tensors(off):
    dev, shape, fill = torch.device("cpu"), (3, 5), 5.0
    g = Guarded(dev, shape, fill, off=off)
    assert g.intact() and g.t.shape == shape and g.full.numel() == off + 15 + SLACK and bool((g.t == fill).all())
    assert g.t.data_ptr() % 16 == (4 * off) % 16 and g.ptr.value == g.t.data_ptr()
    assert g.t.data_ptr() == g.full.data_ptr() + 4 * off
    g.full[off + 15] = 7.0                                  # directly behind
    assert not g.intact()
    g.full[off + 15] = fill
    assert g.intact()
    g.full[-1] = 7.0                                        # the last guard element
    assert not g.intact()
    g.full[-1] = fill
    if off > 0:
        for at in (off - 1, 0):                             # directly in front, and the first guard element
            g.full[at] = 7.0
            assert not g.intact()
            g.full[at] = fill
    g.t.fill_(-1.0)                                         # the tensor itself is not guarded
    assert g.intact()
    b = Guarded(dev, shape, fill, off=off, body=float("nan"))
    assert bool(torch.isnan(b.t).all()) and b.intact() and int(torch.isnan(b.full).sum()) == 15
    init = torch.arange(15, dtype=torch.float32).view(shape)
    for given in (init, init.numpy()):
        i = Guarded(dev, shape, fill, given, off, body=0.5)     # init goes before body
        assert torch.equal(i.t, init) and i.intact() and i.host().tolist() == init.tolist()
    u = Guarded(dev, shape, 7, off=off if off != 1 else 0, dtype=torch.uint8)
    assert u.full.dtype == torch.uint8 and u.intact()


def _modules():
    for path in sorted(glob.glob(os.path.join(TESTS, "*.py"))):
        yield os.path.basename(path), ast.parse(open(path).read(), path)


def test_no_module_imports_a_test_module():
    """At module level or inside a function."""
    found = []
    for name, tree in _modules():
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                mods = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                mods = [node.module or ""]
            else:
                continue
            found += [(name, node.lineno, m) for m in mods if m.split(".")[-1].startswith("test_") or m.split(".")[0].startswith("test_")]
    assert not found, found


def test_guarded_is_defined_once():
    where = [name for name, tree in _modules() for node in ast.walk(tree) if isinstance(node, ast.ClassDef) and node.name == "Guarded"]
    assert where == ["guarded.py"], where


def test_no_test_module_defines_the_dev_fixture():
    where = [name for name, tree in _modules() if name.startswith("test_")
             for node in ast.walk(tree) if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) and node.name == "dev"]
    assert not where, where
    support = dict(_modules())["support.py"]
    assert [n.name for n in support.body if isinstance(n, ast.FunctionDef) and n.name == "dev"] == ["dev"]
