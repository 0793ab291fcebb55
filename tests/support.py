"""What every test module may take for granted: the `dev` fixture of the GPU tests, the NumPy -> torch handle `T`, the bit view
`bits`, and the one-line configuration `cfg_of` of the CPU tests.  Test modules import from here and from the harness and cases
modules beside it, never from one another (tests/test_support_cpu.py holds that rule)."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def cfg_of(algo, *extra):
    from pql_amd.utils.cfg import load_cfg
    return load_cfg([f"algo={algo}", "task.name=Toy", "num_envs=4", *extra])


def child_env(**extra):
    """The environment of a child python that imports pql_amd and the modules beside this one: both folders in front of PYTHONPATH."""
    path = [os.path.join(ROOT, "tests"), ROOT, *filter(None, os.environ.get("PYTHONPATH", "").split(os.pathsep))]
    return dict(os.environ, PYTHONPATH=os.pathsep.join(path), **extra)
