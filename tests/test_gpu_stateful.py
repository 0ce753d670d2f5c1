"""The GPU twins of tests/test_operator_stateful.py: the same machines on the product's own HIP backend (DEV = "cuda", BACKEND = None, as
tests/test_gpu_round6.py does for one sequence) for {float16, bfloat16} x {W8, W4} - fixed_sequence, fixed_sequence_ext (whose asserts say
which states were reached) and three seeded sequences of 24 steps each, drawn with random.Random(seed) over the same rules: no hypothesis
on the GPU, so a failure message carries the seed and the steps so far.  Every step: the block with every caching feature on returns the
bytes of the twin that keeps nothing, and holds the same reference-visible state.  Tiny shapes (K = 128 / 256, I = 64, at most 24 rows),
one synchronize per forward, no graph capture (the module tests cover it)."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_operator_stateful as S  # noqa: E402
from mixq_amd import _capi  # noqa: E402

SEEDS = (1, 2, 3)
STEPS = 24


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    assert "gfx950" in _capi.device_info()
    lib = _capi.load()
    lib.mixq_gemm_set_config(-1); lib.mixq_gemm_w8a16_set_config(-1)
    yield


def on_gpu(cls):
    return type(cls.__name__ + "Gpu", (cls,), {"DEV": "cuda", "BACKEND": None})


@pytest.mark.parametrize("cls", S.MACHINES, ids=lambda c: c.__name__)
def test_fixed_sequence_on_gpu(cls):
    S.fixed_sequence(on_gpu(cls)())
    torch.cuda.synchronize()


@pytest.mark.parametrize("cls", S.MACHINES, ids=lambda c: c.__name__)
def test_fixed_sequence_ext_on_gpu(cls):
    S.fixed_sequence_ext(on_gpu(cls)())
    torch.cuda.synchronize()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("cls", S.MACHINES, ids=lambda c: c.__name__)
def test_seeded_sequence_on_gpu(cls, seed):
    rng = random.Random(seed)
    m = on_gpu(cls)()
    done = []
    try:
        m.build(rng.randint(0, 3), warm=rng.random() < 0.5)
        for _ in range(STEPS):
            try:
                done.append(m.random_step(rng))
            except AssertionError as e:
                raise AssertionError(f"{cls.__name__} seed {seed}, after {done}: {e}") from e
        m.same_state_dict()
    finally:
        m.teardown()
    torch.cuda.synchronize()
