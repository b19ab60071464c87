"""libpsnd_hip.so: loads without a GPU, exports every symbol include/psnd.h declares, host-side
entry points (integer framing contract, plan builders, argument validation) behave."""
import ctypes
import os
import re
import numpy as np
import pytest

from conftest import ROOT
from oracle import features as ofe


CTYPE = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
         'uint32_t': ctypes.c_uint32, 'uint64_t': ctypes.c_uint64}


def _header_text(lab=False):
    """include/psnd.h without comments: the product's declarations, or (lab) the inside of the #ifdef PSND_LAB blocks"""
    txt = open(os.path.join(ROOT, 'include', 'psnd.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    if lab:
        return '\n'.join(re.findall(r'#ifdef PSND_LAB(.*?)#endif', txt, flags=re.S))         # lab-only entry points (libpsnd_hip_lab.so)
    return re.sub(r'#ifdef PSND_LAB.*?#endif', '', txt, flags=re.S)


def _declared(lab=False):
    return sorted(set(re.findall(r'\b(psnd_[a-z0-9_]+)\s*\(', _header_text(lab))))


def _prototypes(txt):
    """this file's own reader of the header (nothing of the package's parser): name -> (restype, [argtypes], [argument texts])"""
    out = {}
    txt = re.sub(r'^[ \t]*#.*$', '', txt, flags=re.M)
    for ret, name, arglist in re.findall(r'(\w[\w\s]*?[\s*]+)(psnd_\w+)\s*\(([^()]*)\)\s*;', txt):
        args = [] if arglist.strip() == 'void' else [' '.join(a.split()) for a in arglist.split(',')]
        res = ((ctypes.c_char_p if 'char' in ret else ctypes.c_void_p) if '*' in ret else
               None if ret.strip() == 'void' else CTYPE[ret.strip()])
        out[name] = (res, [ctypes.c_void_p if '*' in a else CTYPE[a.split()[0]] for a in args], args)
    return out


@pytest.fixture(scope='module')
def L():
    from pytorch_sound_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib


def test_exports_every_declared_symbol(L):
    h = ctypes.CDLL(L.LIB_PATH)
    names = _declared()
    assert len(names) >= 12
    for n in names:
        assert hasattr(h, n), 'include/psnd.h declares %s but the library does not export it' % n
    assert sorted(L.SIGNATURES) == names, 'ctypes table and header disagree'
    assert not hasattr(h, 'psnd_env_refresh'), 'the product library exports the lab build\'s switch refresh'
    assert L.lib().psnd_version() >= 100


def test_every_signature_matches_the_header(L):
    """return type, arity and every argument type of every declared function, the lab block included, against the binding's tables"""
    for lab, table in ((False, L.SIGNATURES), (True, L.LAB_SIGNATURES)):
        protos = _prototypes(_header_text(lab))
        assert sorted(protos) == _declared(lab) == sorted(table), 'ctypes table and header disagree'
        for name, (res, argtypes, args) in protos.items():
            assert table[name][0] is res, '%s: return type %s' % (name, table[name][0])
            assert len(table[name][1]) == len(args), '%s: %d arguments bound, %d declared' % (name, len(table[name][1]), len(args))
            for a, want, got in zip(args, argtypes, table[name][1]):
                assert got is want, '%s: `%s` is bound as %s' % (name, a, got)
    assert len(L.SIGNATURES) >= 155 and list(L.LAB_SIGNATURES) == ['psnd_env_refresh']


def test_mirrored_structs_match_the_header(L):
    """the ctypes classes of the header's descriptor structs: same field names in the same order; psnd_wnorm_desc is 7 pointers + 6 ints"""
    bodies = dict(re.findall(r'typedef struct (psnd_\w+) \{(.*?)\} \1;', _header_text(), flags=re.S))
    for name, mirror in (('psnd_wgrad_desc', L.WgradDesc), ('psnd_chain_pair', L.ChainPair), ('psnd_wnorm_desc', L.WnormDesc)):
        declared = [re.search(r'(\w+)\s*$', f).group(1) for decl in bodies[name].split(';') for f in decl.split(',') if f.strip()]
        assert [f for f, _ in mirror._fields_] == declared, name
    assert ctypes.sizeof(L.WnormDesc) == 80                          # x86-64 LP64, the GPU hosts' ABI
    assert ctypes.sizeof(L.WgradDesc) == 56
    assert ctypes.sizeof(L.ChainPair) == 112
    assert [t for _, t in L.WnormDesc._fields_] == [ctypes.c_void_p] * 7 + [ctypes.c_int] * 6


def test_constants_equal_the_header(L):
    """every Python constant that stands for a header macro, against this file's own reading of the #define lines and the pinned literals"""
    from pytorch_sound_amd import kernels as K
    macros = {n: int(v) for n, v in re.findall(r'^#define (PSND_\w+) \(?(-?\d+)\)?\s*$', _header_text(), flags=re.M)}
    assert macros == L.DEFINES
    pinned = dict(PSND_OK=0, PSND_E_ARG=-1, PSND_E_SHAPE=-2, PSND_E_HIP=-3, PSND_E_UNSUPPORTED=-4,
                  PSND_FRAMING_CENTER=0, PSND_FRAMING_HIFIGAN=1, PSND_FRAMING_NONE=2, PSND_LOG_NONE=0, PSND_LOG_E=1, PSND_LOG_10=2,
                  PSND_MASK_NONE=0, PSND_MASK_LINEAR=1, PSND_MASK_SIGMOID=2, PSND_WNORM_MAX=32,
                  PSND_IPREEMPH_SPAN=8192, PSND_IPREEMPH_WARM_MAX=2048, PSND_IPREEMPH_SEQ=-1, PSND_IPREEMPH_AUTO=-2,
                  PSND_LFILTER_SPAN=8192, PSND_LFILTER_CHUNK=32, PSND_LFILTER_PARALLEL=0, PSND_LFILTER_SEQ=1,
                  PSND_RESAMPLE_TILE=1024, PSND_RESAMPLE_MAX_TAPS=12801, PSND_SILENCE_BLOCK=1024)
    assert macros == pinned
    for mod, prefix, names in ((L, 'PSND_', ('PSND_OK', 'FRAMING_CENTER', 'FRAMING_HIFIGAN', 'FRAMING_NONE', 'LOG_NONE', 'LOG_E', 'LOG_10',
                                             'MASK_NONE', 'MASK_LINEAR', 'MASK_SIGMOID')),
                               (K, 'PSND_', ('IPREEMPH_SPAN', 'IPREEMPH_WARM_MAX', 'IPREEMPH_SEQ', 'IPREEMPH_AUTO', 'LFILTER_SPAN',
                                             'LFILTER_PARALLEL', 'LFILTER_SEQ', 'RESAMPLE_TILE', 'RESAMPLE_MAX_TAPS', 'SILENCE_BLOCK'))):
        for n in names:
            assert getattr(mod, n) == macros[n if n.startswith(prefix) else prefix + n], n
    assert 'PSND_GN_WS_DOUBLES' not in L.DEFINES and 'PSND_H' not in L.DEFINES


# ---- the binding's parser refuses what it cannot type (header TEXT in, no library needed) --------------------------------------------------
GOOD = 'int psnd_a(const float *x, int64_t n, void *stream);\n'


@pytest.mark.parametrize('text,offender', [
    (GOOD + 'int psnd_b(long double x, void *stream);\n', 'psnd_b'),                                   # a type word outside the grammar
    (GOOD + 'long psnd_b(int x);\n', 'psnd_b'),                                                        # ... as the return type
    (GOOD + 'typedef struct psnd_s {\n    const void *p, *q;\n    long double w;\n} psnd_s;\n', 'psnd_s'),     # a struct field
    (GOOD + '#define PSND_X (1 << 3)\n', 'PSND_X'),                                                    # not an integer literal
    (GOOD + '#define PSND_Y PSND_OK\n', 'PSND_Y'),
    ('int psnd_b(int x)\n' + GOOD, 'psnd_b'),                                                          # two prototypes run together
    (GOOD + 'int psnd_b(int x)\n', 'psnd_b'),                                                          # the last one left open
    (GOOD + '#if 0\nint psnd_b(int x);\n#endif\n', '#if 0'),                                           # a block it would read as live
])
def test_parser_refuses_what_it_cannot_type(text, offender):
    from pytorch_sound_amd import _lib
    assert list(_lib.parse_header(GOOD)[0]) == ['psnd_a']
    with pytest.raises(_lib.PsndError, match=re.escape(offender)):
        _lib.parse_header(text)


def test_parser_refuses_the_real_header_with_a_semicolon_removed():
    from pytorch_sound_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'psnd.h')).read()
    sigs, lab, structs, defines = _lib.parse_header(txt)
    assert len(sigs) == len(_lib.SIGNATURES) and sorted(structs) == ['psnd_chain_pair', 'psnd_wgrad_desc', 'psnd_wnorm_desc']
    for name in ('psnd_lfilter', 'psnd_version', 'psnd_l1_loss_bwd_w', 'psnd_conv1d_cl_wgrad_multi_splits'):
        m = re.search(r'\b%s\s*\([^()]*\)\s*;' % name, txt)
        broken = txt[:m.end() - 1] + txt[m.end():]
        with pytest.raises(_lib.PsndError, match=name):
            _lib.parse_header(broken)


def test_a_missing_header_is_an_error_that_names_the_path(monkeypatch):
    from pytorch_sound_amd import _lib
    monkeypatch.setattr(_lib, 'HEADER_PATH', '/nonexistent/include/psnd.h')
    with pytest.raises(_lib.PsndError, match='/nonexistent/include/psnd.h'):
        _lib._read_header()


# ---- the launcher (_lib.on) serves the entry points that take a stream, and only those -------------------------------------------------------
def test_launchable_entry_points_are_those_whose_last_parameter_is_the_stream(L):
    """against a regex of this file's own over the header text (the lab block included)"""
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'psnd.h')).read(), flags=re.S)
    want = set(re.findall(r'\b(psnd_\w+)\s*\([^()]*\bvoid\s*\*\s*stream\s*\)\s*;', txt))
    assert len(want) >= 100 and want == set(L.LAUNCHABLE)
    for name in ('psnd_frame_count', 'psnd_stft_plan_bytes', 'psnd_last_error', 'psnd_stream_wait_event'):
        assert name in L.SIGNATURES and name not in L.LAUNCHABLE
    assert all(L.SIGNATURES[n][0] is ctypes.c_int and L.SIGNATURES[n][1][-1] is ctypes.c_void_p for n in L.LAUNCHABLE & set(L.SIGNATURES))
    assert 'psnd_a' not in L.LAUNCHABLE                          # parsing other header text leaves the module's set alone
    streamed = set()
    L.parse_header(GOOD + 'int psnd_b(void *stream, int x);\nvoid psnd_c(void *stream);\n', streamed)
    assert streamed == {'psnd_a'}


def test_launcher_resolves_names_without_entering(L):
    k = L.on(0)                                                  # not entered: no device is touched
    with pytest.raises(AttributeError, match='psnd_no_such_entry'):
        k.psnd_no_such_entry
    with pytest.raises(L.PsndError, match='psnd_stft_plan_bytes'):
        k.psnd_stft_plan_bytes
    assert not hasattr(k, 'psnd_no_such_entry')
    assert callable(k.psnd_stft_fwd)


def test_frame_contract_matches_oracle(L):
    lib = L.lib()
    for T, n, h in [(44100, 1024, 256), (8192, 1024, 256), (1323000, 4096, 1024), (700, 256, 64), (2049, 1024, 255),
                    (513, 1024, 256), (100, 1024, 256)]:
        for framing in (0, 1):
            F = ofe.frame_count(T, n, h, framing)
            assert lib.psnd_frame_count(T, n, h, framing) == F
            if T <= ofe.pad_amount(n, h, framing):
                continue
            for f in sorted({0, 1, 2, F // 2, max(F - 2, 0), max(F - 1, 0)}):
                ms = np.array([0, 1, n // 2 - 1, n // 2, n - 1])
                want = ofe.frame_sample_index(f, ms, T, n, h, framing)
                got = [lib.psnd_frame_sample_index(f, int(m), T, n, h, framing) for m in ms]
                assert list(want) == got


def test_plans_build_on_host(L):
    for n in (64, 256, 512, 1024, 2048, 4096):
        w = ofe.analysis_window(n)
        plan = L.build_stft_plan(n, w)
        assert plan.nbytes == L.lib().psnd_stft_plan_bytes(n) > 0
        pf = plan.view(np.float32)
        raw = pf[:n] if n in (64, 4096) else pf[-2 * n:-n]            # generic sizes lead with it, tuned ones append a permuted copy
        assert np.array_equal(raw, w)                                # the raw window is in every plan
    assert L.lib().psnd_stft_plan_bytes(1000) == 0                   # not a power of two
    W = ofe.mel_filterbank(22050, 1024, 80, 0, 8000)
    mp = L.build_mel_plan(W).view(np.int32)
    assert list(mp[:6]) == [80, 513, 5, 129, 33, 20]
    bands = mp[8:8 + 10].reshape(5, 2)
    nz = [np.nonzero(W[16 * t:16 * t + 16].sum(0))[0] for t in range(5)]
    for t in range(5):
        assert bands[t, 0] == nz[t].min() // 4 and bands[t, 1] == nz[t].max() // 4 + 1
    assert (bands[:, 1] - bands[:, 0]).sum() < 0.25 * 5 * 129        # band sparsity is real


def test_argument_validation_without_gpu(L):
    lib = L.lib()
    assert lib.psnd_stft_fwd(None, 1, 100, 1024, 256, 0, None, 0.0, None, None, None, None, None) == -1
    assert b'null' in lib.psnd_last_error()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.psnd_stft_fwd(p, 1, 100, 1024, 256, 0, p, 0.0, p, None, None, None, None) == -2     # T <= pad
    assert lib.psnd_stft_fwd(p, 1, 5000, 1000, 256, 0, p, 0.0, p, None, None, None, None) == -4    # n_fft unsupported
    assert lib.psnd_stft_fwd(p, 1, 5000, 1024, 256, 7, p, 0.0, p, None, None, None, None) == -1    # framing enum
    assert lib.psnd_mel_fwd(None, 1, 1, 80, 513, None, 1, 0.0, -1.0, 0.0, 0.0, None, None, None) == -1
    assert lib.psnd_stft_bwd(p, 1, 5000, 1024, 256, 0, p, 0.0, None, None, None, p, None) == -1    # no gradient source


def test_argument_validation_of_the_wider_entry_points(L):
    """every entry point added behind the feature path rejects bad arguments before touching the device (0 work sizes are OK)"""
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.psnd_preemphasis_fwd(p, 1, 1, 0.97, p, None) == -2                      # reflect pad needs T >= 2
    assert lib.psnd_preemphasis_fwd(None, 1, 8, 0.97, p, None) == -1
    assert lib.psnd_stft_loss_blocks(0) == 0 and lib.psnd_stft_loss_blocks(8192) == 1 and lib.psnd_stft_loss_blocks(8193) == 2
    assert lib.psnd_stft_loss_partial(p, p, 0, 10, 1e-5, p, None) == 0               # empty batch: nothing to do
    assert lib.psnd_stft_loss_final(p, p, 9, 1, p, p, None) == -1                    # more than 8 resolutions
    assert lib.psnd_l1_loss_blocks(16384) == 1 and lib.psnd_l1_loss_blocks(16385) == 2
    assert lib.psnd_l1_loss_fwd(p, p, 0, p, p, None) == -2
    assert lib.psnd_pad_collate(p, p, p, 0, 100, p, None, None) == 0
    assert lib.psnd_pad_collate(p, p, p, 70000, 100, p, None, None) == -2
    assert lib.psnd_pqmf_analysis(p, p, 1, 64, 4, 61, 0, 1.0, p, None) == -2           # odd tap count
    assert lib.psnd_pqmf_analysis(p, p, 1, 64, 17, 62, 0, 1.0, p, None) == -2          # too many subbands
    assert lib.psnd_pqmf_synthesis(p, p, 0, 16, 64, 4, 62, 0, 4.0, p, None) == 0
    assert lib.psnd_adam_step(p, 1, p, p, 1, 1e-3, 1.0, 0.999, 1e-8, 0.0, 0, None, None, p, 0.0, None, None) == -1    # beta1 = 1
    assert lib.psnd_adam_step(p, 1, p, p, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None, None, p, -1.0, None, None) == -1   # clip_value < 0
    assert lib.psnd_grad_sumsq(p, 1, p, p, 1, 0.0, None, 0, 1.0, None, p, p, None) == -1                              # no scratch
    assert lib.psnd_grad_sumsq(p, 1, p, p, 1, 0.0, None, 0, -1.0, p, p, p, None) == -1                                # max_norm < 0
    assert lib.psnd_polar_bwd(None, None, p, p, 4, p, p, None) == -1                                                   # no gradient given
    assert lib.psnd_adam_step(p, 0, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None, None, p, 0.0, None, None) == 0
    assert lib.psnd_adam_chunk() == 2048 and lib.psnd_adam_table_bytes() == 48
    assert lib.psnd_conv1d_wnorm_bwd_multi(p, 0, None) == -1 and lib.psnd_conv1d_wnorm_bwd_multi(p, 33, None) == -1
    assert lib.psnd_mask_head_fwd(None, p, 1, 8, 8, 8, 0, 32, p, None) == -1
    assert lib.psnd_conv1d_cl(p, None, None, 0.0, p, None, None, None, 1, 16, 8, 4, 32, 40, 3, -1, 1, 0.1, 1.0, p, None, None, None) == -2   # Cb % 32


def test_product_has_no_fallback(L, monkeypatch):
    """a CPU tensor or a missing library must raise, never compute on the host."""
    import torch
    from pytorch_sound_amd import kernels
    with pytest.raises(L.PsndError):
        kernels.stft_forward(torch.zeros(1, 4096), 1024, 256, torch.zeros(8, dtype=torch.uint8))
    monkeypatch.setattr(L, '_lib', None)
    monkeypatch.setattr(L, 'LIB_PATH', '/nonexistent/libpsnd_hip.so')
    with pytest.raises(L.PsndError):
        L.lib()
