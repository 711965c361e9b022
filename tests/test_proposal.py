"""
What a target sees from the three samplers that use the fitted map as their proposal: the first call of log_target_pdf in
sample_importance, sample_mcmc and sample_smc gets, bit for bit, the rows of sample(N, X_star, seed, draw0) - the raw
coordinates as the export kernel rounds them (x * sd + mean, two roundings), whether the target runs on the host (NumPy rows)
or on the device (a (columns, N) tensor).  sample_importance hands over every returned column, the chain and particle drivers
the own columns behind the E conditioning ones.  On the host test double and on the GPU; N is odd, so the padding column of
the device matrices exists.  A GPU process never loads the host double.
"""
import numpy as np
import pytest

from tests.hostemu import emu
from tests.test_mcmc import FORCED_CASES, bits, make, same_bits

N, SEED, DRAW0 = 301, 13, 20
CASES = FORCED_CASES + [('c3_sep', dict(standardize_samples=False), 0)]
IDS = ['c3_sep', 'c5_sep_newton_one_point', 'c2a_int', 'c3_sep_unstandardized']


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


class Recording:
    """The mild target -0.5e-3 |x|^2 in either convention; keeps a copy, as N rows, of what its first call was given."""

    def __init__(self, on_device):
        self.on_device, self.first, self.calls = on_device, None, 0

    def __call__(self, x):
        self.calls += 1
        if self.on_device:
            if self.first is None:
                self.first = np.ascontiguousarray(x.detach().cpu().numpy().T).copy()
            return -0.5e-3 * (x * x).sum(dim=0)
        if self.first is None:
            self.first = np.array(x, dtype=float, copy=True)
        return -0.5e-3 * np.sum(x * x, axis=1)


def run(tm, driver, target, X_star, on_device):
    if driver == 'importance':
        tm.sample_importance(N, target, X_star=X_star, seed=SEED, draw=DRAW0, target_on_device=on_device)
    elif driver == 'mcmc':
        tm.sample_mcmc(target, N, 2, X_star=X_star, seed=SEED, draw=DRAW0, target_on_device=on_device)
    else:
        tm.sample_smc(target, N, X_star=X_star, moves=1, seed=SEED, draw=DRAW0, target_on_device=on_device)


@pytest.mark.parametrize('on_device', [False, True], ids=['host_target', 'device_target'])
@pytest.mark.parametrize('driver', ['importance', 'mcmc', 'smc'])
@pytest.mark.parametrize('name,override,E', CASES, ids=IDS)
def test_the_first_call_of_the_target_sees_the_draws_of_sample(backend, name, override, E, driver, on_device):
    tm, Xtrain = make(name, **override)
    X_star = np.asarray(Xtrain[3, :E], dtype=float) if E else None
    want = tm.sample(N, X_star=X_star, seed=SEED, draw=DRAW0)
    if driver != 'importance':
        want = want[:, E:]
    target = Recording(on_device)
    run(tm, driver, target, X_star, on_device)
    assert target.calls >= 1 and target.first is not None
    saw = target.first
    differ = np.flatnonzero(np.any(bits(saw) != bits(want), axis=1))[:8].tolist() if saw.shape == want.shape else 'all (shape)'
    print('%s %s %s %s: the target saw %s, sample() gives %s, rows that differ: %s'
          % (backend, name, driver, 'device' if on_device else 'host', saw.shape, want.shape, differ))
    assert same_bits(saw, want)
