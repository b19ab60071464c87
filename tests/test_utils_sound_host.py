"""pytorch_sound.utils.sound without a GPU: the alias import, the numpy paths against the golden fixture of the reference, the CPU-tensor
paths against the float64 yardstick (tests/lfilter_ref.py), cookbook known answers of the biquads, the host rule that picks the kernel
instance, argument errors, the two C ABI entries, and autograd on the CPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import signal

import lfilter_ref as R
from conftest import ROOT


@pytest.fixture(scope='module')
def snd():
    import pytorch_sound.utils.sound as m
    return m


@pytest.fixture(scope='module')
def L():
    from pytorch_sound_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib


def test_alias_import_is_the_same_module():
    import pytorch_sound.utils.sound as a
    import pytorch_sound_amd.utils.sound as b
    from pytorch_sound.utils.sound import preemphasis, inv_preemphasis, lowpass, get_wav_duration  # noqa: F401
    assert a is b
    for absent in ('parse_midi', 'get_f0'):
        assert not hasattr(a, absent) and absent in a.__doc__


@pytest.mark.parametrize('tag,coeff', [('0p97', 0.97), ('0p5', 0.5)])
def test_numpy_paths_equal_the_reference_bit_for_bit(snd, golden, tag, coeff):
    g = golden('utils_sound')
    x = g['x']
    assert x.shape == (2, 4099) and x.dtype == np.float32
    for name in ('preemphasis', 'inv_preemphasis'):
        got = getattr(snd, name)(x, coeff)
        want = g['%s_%s' % (name, tag)]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), name
    assert np.array_equal(snd.preemphasis(x), g['preemphasis_0p97'])               # the default coefficient


@pytest.mark.parametrize('name', sorted(R.FILTERS))
@pytest.mark.parametrize('reverse', [False, True])
def test_cpu_tensor_paths_are_within_the_bound(name, reverse):
    from pytorch_sound_amd import kernels as K
    b, a = R.FILTERS[name]
    x = R.signal_rows(3, 3, 8193)
    got = K.lfilter(torch.from_numpy(x), b, a, reverse=reverse)
    assert got.dtype == torch.float32 and got.shape == (3, 8193)
    assert R.excess(got.numpy(), R.reference(x, b, a, reverse)) <= 1.0


def test_cpu_tensor_dtypes_shapes_and_the_module_functions(snd, golden):
    g = golden('utils_sound')
    x = torch.from_numpy(g['x'])
    for name, tag in (('preemphasis', 'preemphasis_0p97'), ('inv_preemphasis', 'inv_preemphasis_0p97')):
        got = getattr(snd, name)(x)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.device == x.device
        assert R.excess(got.numpy(), g[tag].astype(np.float64), scale=2.0) <= 1.0      # the golden is itself a float32 rounding
    assert snd.lowpass(x.double(), 100).dtype == torch.float64
    assert snd.lowpass(x.to(torch.bfloat16), 100).dtype == torch.bfloat16
    assert snd.highpass(x.reshape(2, 1, 4099), 80).shape == (2, 1, 4099)
    assert snd.biquad(x[0], [1.0], [1.0, -0.5]).shape == (4099,)
    assert snd.biquad(x[:, :0], [1.0], [1.0, -0.5]).shape == (2, 0)
    y = snd.biquad(x.t().contiguous().t(), [1.0], [1.0, -0.5])                         # a non-contiguous view
    assert torch.equal(y, snd.biquad(x, [1.0], [1.0, -0.5]))


def test_inverse_preemphasis_undoes_preemphasis(snd, golden):
    x = golden('utils_sound')['x']
    assert np.abs(snd.inv_preemphasis(snd.preemphasis(x)) - x).max() <= 1e-6
    xt = torch.from_numpy(x)
    assert (snd.inv_preemphasis(snd.preemphasis(xt)) - xt).abs().max().item() <= 1e-6
    # models.sound.PreEmphasis reflect-pads one sample: the two differ in sample 0 only
    y0 = snd.preemphasis(x)
    refl = x.copy()
    refl[:, 1:] -= 0.97 * x[:, :-1]
    refl[:, 0] -= 0.97 * x[:, 1]
    assert np.abs(y0[:, 1:] - refl[:, 1:]).max() <= 1e-7 and np.abs(y0[:, 0] - x[:, 0]).max() == 0


def test_lowpass_known_answers(snd):
    """Audio EQ Cookbook: DC gain 1; |H(f0)| = q, i.e. -3.01 dB at the cutoff for q = 0.707; and the low-pass and the high-pass of one
    signal add up to an all-pass magnitude in power, |H_lp|^2 + |H_hp|^2 = 1.  With u = cos w, c = cos w0 the numerators give
    (1 - c)^2 (1 + u)^2 + (1 + c)^2 (1 - u)^2 = 2 (1 + c^2)(1 + u^2) - 8 c u, and the shared denominator 4 (u - c)^2 + 4 alpha^2 (1 - u^2) is
    the same expression exactly when alpha^2 = sin^2 w0 / 2, q = 1 / sqrt 2.  q = 0.707 is 1.5e-4 short of that, alpha^2 off by 3e-4
    relative: the power sum stays within 3e-4 of 1, asserted at 1e-3.  (The plain sum H_lp + H_hp is a notch at f0, not an all-pass.)"""
    for f, fs in ((100, 44100), (1000, 44100), (3000, 22050)):
        b, a = snd.lowpass_coefficients(f, fs)
        bh, ah = snd.highpass_coefficients(f, fs)
        assert ah == a
        assert abs(sum(b) / sum(a) - 1.0) <= 1e-12 and abs(sum(bh)) <= 1e-12            # DC: 1 and 0
        alt = lambda c: sum(v * (-1) ** i for i, v in enumerate(c))                     # noqa: E731 - the response at Nyquist
        assert abs(alt(bh) / alt(a) - 1.0) <= 1e-12 and abs(alt(b)) <= 1e-12
        _, h = signal.freqz(b, a, [f], fs=fs)
        db = 20 * np.log10(abs(h[0]))
        assert abs(db - 20 * np.log10(0.707)) <= 1e-9 and abs(db + 3.01) <= 0.01
        w = np.linspace(10, fs / 2 - 10, 257)
        _, hl = signal.freqz(b, a, w, fs=fs)
        _, hh = signal.freqz(bh, ah, w, fs=fs)
        assert np.abs(np.abs(hl) ** 2 + np.abs(hh) ** 2 - 1.0).max() <= 1e-3
    # on one signal: the two halves of white noise carry its energy between them (Parseval; the tails cut at T are the 2e-3)
    x = R.signal_rows(9, 1, 1 << 16)[0]
    for inp in (x, torch.from_numpy(x)):
        lo, hi = (np.asarray(v, dtype=np.float64) for v in (snd.lowpass(inp, 1000), snd.highpass(inp, 1000)))
        assert abs((np.sum(lo ** 2) + np.sum(hi ** 2)) / np.sum(x.astype(np.float64) ** 2) - 1.0) <= 2e-3
    # a step settles to the step behind the low-pass and to zero behind the high-pass
    one = np.ones(20000, dtype=np.float32)
    lo, hi = snd.lowpass(one, 200), snd.highpass(one, 200)
    assert lo.dtype == np.float32 and abs(lo[-1] - 1.0) <= 1e-6 and abs(hi[-1]) <= 1e-6
    assert np.abs(snd.lowpass(torch.from_numpy(one), 200).numpy() - lo).max() <= 1e-6


def test_wav_duration(snd, tmp_path):
    from scipy.io import wavfile
    path = str(tmp_path / 'a.wav')
    wavfile.write(path, 8000, np.zeros(12000, dtype=np.int16))
    assert snd.get_wav_duration(path) == 1.5
    assert snd.get_wav_duration(str(tmp_path / 'missing.wav')) == -1                   # as the reference: -1 on any failure


def _radius_pair(r):
    """a second-order denominator with a complex pole pair of radius r"""
    return [1.0, -2 * r * np.cos(0.3), r * r]


@pytest.mark.parametrize('a,want', [([1.0, -0.97], 'parallel'), (_radius_pair(0.97), 'parallel'), (_radius_pair(0.998), 'parallel'),
                                    ([1.0, -1.0], 'parallel'), (_radius_pair(1.0), 'parallel'), ([1.0, -1.001], 'parallel'),
                                    ([1.0, -1.2], 'seq'), (_radius_pair(1.2), 'seq'), ([1.0, float('nan')], 'seq'),
                                    ([2.0, -2.4], 'seq'), ([1.0], 'parallel')])
def test_instance_rule_against_brute_force(a, want):
    from pytorch_sound_amd import kernels as K
    got = K.lfilter_instance([1.0], a)
    assert got == {'parallel': K.LFILTER_PARALLEL, 'seq': K.LFILTER_SEQ}[want]
    an = (np.asarray(a, dtype=np.float64) / a[0]).tolist() + [0.0, 0.0]
    with np.errstate(all='ignore'):
        P = np.linalg.matrix_power(np.array([[-an[1], 1.0], [-an[2], 0.0]]), K.LFILTER_SPAN)
    assert (got == K.LFILTER_PARALLEL) == bool(np.isfinite(P).all())
    assert K.lfilter_instance([float('nan')], [1.0, -0.5]) == K.LFILTER_SEQ             # a NaN numerator too


def test_argument_errors(snd):
    from pytorch_sound_amd import kernels as K
    x = torch.zeros(2, 8)
    with pytest.raises(ValueError):
        K.lfilter(x, [1.0], [0.0, 1.0])
    with pytest.raises(ValueError):
        snd.biquad(np.zeros(8, dtype=np.float32), [1.0], [0.0, 1.0])
    for b, a in (([1.0, 2.0, 3.0, 4.0], [1.0]), ([1.0], [1.0, 0.1, 0.1, 0.1]), ([], [1.0])):
        with pytest.raises(K.PsndError, match='order <= 2'):
            K.lfilter(x, b, a)
    with pytest.raises(K.PsndError, match='order <= 2'):
        snd.biquad(np.zeros(8, dtype=np.float32), [1.0, 2.0, 3.0, 4.0], [1.0])
    with pytest.raises(K.PsndError):
        K.lfilter(torch.zeros(()), [1.0], [1.0])
    with pytest.raises(K.PsndError):
        K.lfilter(x, [1.0], [1.0], instance=7)
    assert K.lfilter_section([2.0], [2.0, 1.0]) == (1.0, 0.0, 0.0, 0.5, 0.0)


def test_abi_symbols_are_exported_declared_and_mirrored(L):
    txt = open(os.path.join(ROOT, 'include', 'psnd.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    h = ctypes.CDLL(L.LIB_PATH)
    for name, ret, last in (('psnd_lfilter', 'int', ['reverse', 'instance', 'carry', 'y', 'stream']), ('psnd_lfilter_spans', 'int64_t', ['T'])):
        m = re.search(r'%s\s+%s\s*\((.*?)\)\s*;' % (ret, name), txt, flags=re.S)
        assert m, 'include/psnd.h does not declare %s' % name
        args = [s.strip() for s in m.group(1).split(',')]
        names = [re.search(r'(\w+)$', s).group(1) for s in args]
        assert names[-len(last):] == last
        assert hasattr(h, name)
        res, argtypes = L.SIGNATURES[name]        # every argument type: tests/test_cabi.py, test_every_signature_matches_the_header
        assert res is (ctypes.c_int if ret == 'int' else ctypes.c_int64) and len(argtypes) == len(args)
    for macro, value in (('PSND_LFILTER_SPAN', 8192), ('PSND_LFILTER_CHUNK', 32), ('PSND_LFILTER_PARALLEL', 0), ('PSND_LFILTER_SEQ', 1)):
        assert re.search(r'#define %s %d\b' % (macro, value), txt), macro
    from pytorch_sound_amd import kernels as K
    assert (K.LFILTER_SPAN, K.LFILTER_PARALLEL, K.LFILTER_SEQ) == (8192, 0, 1)
    assert L.lib().psnd_version() >= 144


def test_bad_arguments_are_refused_without_a_device(L):
    lib = L.lib()
    buf, buf2, cbuf = (ctypes.c_float * 64)(), (ctypes.c_float * 64)(), (ctypes.c_double * 64)()
    x, y, c = (ctypes.cast(v, ctypes.c_void_p) for v in (buf, buf2, cbuf))
    assert [lib.psnd_lfilter_spans(t) for t in (-5, 0, 1, 8192, 8193, 3 * 8192 + 5)] == [0, 0, 1, 1, 2, 4]

    def call(x=x, N=1, T=16, reverse=0, instance=0, carry=c, y=y):
        return lib.psnd_lfilter(x, N, T, 1.0, 0.0, 0.0, -0.97, 0.0, reverse, instance, carry, y, None)

    assert call(carry=None) == -1 and b'carry' in lib.psnd_last_error()
    assert call(N=-1) == -1 and call(T=-1) == -1
    assert call(x=None) == -1 and call(y=None) == -1
    assert call(y=x) == -1 and b'different' in lib.psnd_last_error()
    assert call(instance=2) == -1 and call(instance=-1) == -1 and call(reverse=2) == -1
    assert call(N=1 << 31, T=16) == -2 and call(N=1 << 20, T=1 << 26) == -2            # more than 2^31 - 1 workgroups
    # nothing to do is fine and launches nothing - but the arguments are still checked
    assert call(N=0) == 0 and call(T=0) == 0 and call(N=0, carry=None, x=None, y=None) == 0
    assert call(N=0, instance=5) == -1 and call(T=0, N=-2) == -1


def test_cpu_autograd_is_the_adjoint():
    from pytorch_sound_amd import kernels as K
    g0 = torch.Generator().manual_seed(5)
    for name in ('pole+0.97', 'lowpass100', 'fir', 'integrator'):
        b, a = R.FILTERS[name]
        x = torch.randn(2, 3, 301, dtype=torch.float64, generator=g0, requires_grad=True)
        g = torch.randn(2, 3, 301, dtype=torch.float64, generator=g0)
        y = K.lfilter(x, b, a)
        assert y.dtype == torch.float64
        (gx,) = torch.autograd.grad(y, x, g, create_graph=True)
        want = K.lfilter(g, b, a, reverse=True)
        assert torch.equal(gx, want)
        lhs, rhs = (y.detach() * g).sum().item(), (x.detach() * want).sum().item()
        assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), 1.0)                            # <lfilter(x), g> = <x, lfilter(g, reverse)>
        # second derivative: gx is linear in g, and the gradient of <gx, u> with respect to g is lfilter(u)
        u = torch.randn(2, 3, 301, dtype=torch.float64, generator=g0)
        gg = g.clone().requires_grad_(True)
        (gx2,) = torch.autograd.grad(K.lfilter(x, b, a), x, gg, create_graph=True)
        (d,) = torch.autograd.grad(gx2, gg, u)
        assert torch.equal(d, K.lfilter(u, b, a))
    assert torch.autograd.gradcheck(lambda t: K.lfilter(t, *R.FILTERS['lowpass100']), (torch.randn(1, 40, dtype=torch.float64, requires_grad=True),))
