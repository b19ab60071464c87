"""ctypes binding of libpsnd_hip.so.  include/psnd.h is the only place an entry point, a descriptor struct or a constant is declared: this
module reads it once at import and derives SIGNATURES, LAB_SIGNATURES, the ctypes structs and DEFINES from it (parse_header).  A header
it cannot type completely does not load.  The product path has NO fallback: if the library is missing or a call fails, an exception is
raised."""
import ctypes
import os
import re
import numpy as np
import torch        # before libpsnd_hip.so is loaded (lib), and the base of the launcher's device guard (on)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PSND_LIB', os.path.join(_HERE, 'libpsnd_hip.so'))   # PSND_LIB: A/B builds of the same ABI
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'psnd.h')

_P = ctypes.c_void_p
_lib = None


class PsndError(RuntimeError):
    pass


# ---- the header's grammar: anything with a `*` is a pointer, these are the scalars and the return types -----------------------------------
_SCALARS = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
            'uint32_t': ctypes.c_uint32, 'uint64_t': ctypes.c_uint64}
_RETURNS = {'void': None, 'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'void *': _P,
            'const char *': ctypes.c_char_p}


def _scalar(words, decl):
    if len(words) != 1 or words[0] not in _SCALARS:
        raise PsndError('include/psnd.h: type `%s` of `%s` is outside the binding\'s grammar' % (' '.join(words), decl))
    return _SCALARS[words[0]]


def _prototypes(text, streamed):
    """`ret psnd_name(args);` declarations and nothing else -> {name: (restype, [argtypes])}; the names of those that return an int status
    and whose last parameter is `void *stream` are added to the set `streamed`"""
    *decls, tail = text.split(';')
    if tail.strip():
        raise PsndError('include/psnd.h: `%s` is not closed by a `;`' % ' '.join(tail.split()))
    out = {}
    for decl in (' '.join(d.split()) for d in decls if d.strip()):
        m = re.fullmatch(r'([^()]*?)\b(psnd_\w+) ?\(([^()]*)\)', decl)
        ret = m and re.sub(r' ?\* ?', ' *', m.group(1)).strip()
        if not m or ret not in _RETURNS or m.group(2) in out:
            raise PsndError('include/psnd.h: cannot read `%s` as one prototype of a known return type' % decl)
        args = [] if m.group(3).strip() == 'void' else [a.strip() for a in m.group(3).split(',')]
        out[m.group(2)] = (_RETURNS[ret], [_P if '*' in a else _scalar(a.split()[:-1], decl) for a in args])
        if ret == 'int' and args and re.fullmatch(r'void ?\* ?stream', args[-1]):
            streamed.add(m.group(2))
    return out


def _fields(name, body):
    """the body of `typedef struct name { ... } name;` -> [(field, ctype)], declarators such as `const void *g, *xa;` split"""
    out = []
    for decl in (' '.join(d.split()) for d in body.split(';') if d.strip()):
        first, *more = [p.strip() for p in decl.split(',')]
        base = first.replace('*', ' ').split()[:-1]
        for p in [first] + more:
            field = re.search(r'\w+$', p)
            if not field:
                raise PsndError('include/psnd.h: cannot read field `%s` of %s' % (decl, name))
            out.append((field.group(0), _P if '*' in p else _scalar(base, '%s: %s' % (name, decl))))
    return out


def parse_header(text, streamed=None):
    """the text of include/psnd.h -> (signatures, lab signatures, {struct: [(field, ctype)]}, {macro: int}); raises PsndError on anything
    outside the grammar instead of skipping it.  streamed: a set that receives the names of the entry points that launch on a stream"""
    streamed = set() if streamed is None else streamed
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    defines = {}
    for name, params, body in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(\w+)(\(?)([^\n]*)', text, flags=re.M):
        m = re.fullmatch(r'(-?\d+)|\(\s*(-?\d+)\s*\)', body.strip())
        if m:
            defines[name] = int(m.group(1) or m.group(2))
        elif not params and body.strip():             # the include guard has no body; function-like macros are left to C
            raise PsndError('include/psnd.h: `#define %s %s` is not an integer literal' % (name, body.strip()))
    text = re.sub(r'#ifdef __cplusplus.*?#endif', ' ', text, flags=re.S)
    lab = ' '.join(re.findall(r'#ifdef PSND_LAB\b(.*?)#endif', text, flags=re.S))
    text = re.sub(r'#ifdef PSND_LAB\b.*?#endif', ' ', text, flags=re.S)
    for line in re.findall(r'^[ \t]*#[^\n]*', text, flags=re.M):
        if not re.match(r'\s*#\s*(include|define|ifndef PSND_H|endif)\b', line):
            raise PsndError('include/psnd.h: `%s`: conditional blocks other than PSND_LAB are outside the binding\'s grammar' % line.strip())
    text = re.sub(r'^[ \t]*#[^\n]*', ' ', text, flags=re.M)
    struct = r'typedef struct (psnd_\w+) \{(.*?)\} \1;'
    structs = {name: _fields(name, body) for name, body in re.findall(struct, text, flags=re.S)}
    return _prototypes(re.sub(struct, ' ', text, flags=re.S), streamed), _prototypes(lab, streamed), structs, defines


def _read_header(streamed=None):
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read(), streamed)
    except OSError as e:
        raise PsndError('include/psnd.h not found at %s (%s): the binding is derived from it' % (HEADER_PATH, e))


# name -> (restype, argtypes) of every entry point / of those of a -DPSND_LAB build only; struct -> fields; PSND_* macro -> value
LAUNCHABLE = set()          # the entry points `on` serves: int psnd_name(..., void *stream)
SIGNATURES, LAB_SIGNATURES, _STRUCTS, DEFINES = _read_header(LAUNCHABLE)


def _struct(name):
    return type(''.join(w.capitalize() for w in name.split('_')[1:]), (ctypes.Structure,),
                {'_fields_': _STRUCTS[name], '__doc__': '%s of include/psnd.h' % name})


WgradDesc = _struct('psnd_wgrad_desc')
ChainPair = _struct('psnd_chain_pair')
WnormDesc = _struct('psnd_wnorm_desc')

PSND_OK = DEFINES['PSND_OK']
FRAMING_CENTER, FRAMING_HIFIGAN, FRAMING_NONE = (DEFINES['PSND_FRAMING_' + n] for n in ('CENTER', 'HIFIGAN', 'NONE'))
LOG_NONE, LOG_E, LOG_10 = (DEFINES['PSND_LOG_' + n] for n in ('NONE', 'E', '10'))
MASK_NONE, MASK_LINEAR, MASK_SIGMOID = (DEFINES['PSND_MASK_' + n] for n in ('NONE', 'LINEAR', 'SIGMOID'))


def lib():
    """Load (once) and return the ctypes handle.  Raises if the HIP extension is absent."""
    global _lib
    if _lib is None:
        # torch bundles its own libamdhip64: it must be in the process BEFORE our library is
        # dlopen'ed, otherwise the dynamic linker binds us to a second HIP runtime (/opt/rocm) that
        # never sees torch's device context ("no ROCm-capable device is detected").  This module imports torch at its top.
        if not os.path.exists(LIB_PATH):
            raise PsndError('libpsnd_hip.so not found at %s - run `python -m pytorch_sound_amd._build` '
                            '(there is no CPU / eager fallback)' % LIB_PATH)
        _lib = _load(LIB_PATH)
    return _lib


def _load(path):
    h = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(h, name)       # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in LAB_SIGNATURES.items():     # entry points of a -DPSND_LAB build only
        fn = getattr(h, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    return h


LAB_LIB_PATH = os.path.join(_HERE, 'libpsnd_hip_lab.so')     # `python -m pytorch_sound_amd._build --lab`


def is_lab() -> bool:
    """True when the loaded library is a lab build (reads PSND_* A/B switches from the environment)"""
    return hasattr(lib(), 'psnd_env_refresh')


def refresh_switches():
    """lab build: have the PSND_* switches looked up again after the environment changed; product build: nothing to refresh"""
    if _lib is not None and hasattr(_lib, 'psnd_env_refresh'):
        _lib.psnd_env_refresh()


class use_library:
    """context manager: route every call of this process through another build of the same ABI (the lab library in parity tests of kernel
    instances, tools/ A/B runs) and back.  Plans and tensors are plain memory: they carry over."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        global _lib
        lib()
        if not os.path.exists(self.path):
            raise PsndError('%s not found - run `python -m pytorch_sound_amd._build --lab`' % self.path)
        self.prev, _lib = _lib, _load(self.path)
        return _lib

    def __exit__(self, *exc):
        global _lib
        _lib = self.prev
        return False


def check(rc, what):
    if rc != PSND_OK:
        msg = lib().psnd_last_error()
        raise PsndError('%s failed (%d): %s' % (what, rc, msg.decode() if msg else '?'))


def ptr(t):
    """device (or host) pointer of a contiguous torch tensor, or NULL for None."""
    if t is None:
        return None
    return _P(t.data_ptr())


def np_ptr(a):
    return _P(a.ctypes.data)


def stream_ptr(device):
    return _P(torch.cuda.current_stream(device).cuda_stream)


class on(torch.cuda.device):
    """the one launch path from Python to the library:

        with on(x.device) as hip:
            hip.psnd_posenc(x, pe, scale, N, C, T, Tp, y)

    Entering makes `device` current as torch.cuda.device does and takes that device's current stream ONCE - the side stream under
    torch.cuda.stream(side), the capture stream during a hipGraph capture - so a block never spans a change of the current stream: open a
    nested `on` inside the torch.cuda.stream block instead.  hip.psnd_name(*args) calls that entry point of the library loaded at that
    moment (use_library is followed) with the stream appended, and raises PsndError on a non-zero status.  Where include/psnd.h types a
    parameter as a pointer a tensor becomes its data_ptr(); None (NULL), ctypes objects and int addresses pass as they are.  Only the entry
    points of LAUNCHABLE are served: the others (psnd_*_bytes, plan builders ...) take no stream and are called as lib().psnd_name(...)."""

    def __enter__(self):
        super().__enter__()
        self.stream = torch.cuda.current_stream().cuda_stream
        return self

    def __getattr__(self, name):            # reached only by names that are no launch method (_launch_method, below)
        if name in SIGNATURES or name in LAB_SIGNATURES:
            raise PsndError('%s takes no stream: call it as lib().%s(...)' % (name, name))
        raise AttributeError('%s is not an entry point of include/psnd.h that `on` serves' % name)


def _launch_method(name):
    """on.psnd_name: a plain method, so that a launch costs one attribute lookup and one Python call.  The pointer positions are worked out
    here, once; the handle keeps the functions it has looked up (ctypes); ctypes gets plain ints."""
    argtypes = (SIGNATURES.get(name) or LAB_SIGNATURES[name])[1]
    n = len(argtypes) - 1
    pointers = [i for i in range(n) if argtypes[i] is _P]

    def launch(self, *args):
        fn = getattr(lib(), name)       # of the handle loaded now (use_library swaps it); AttributeError: a lab entry point, a product build
        if len(args) != n:
            raise TypeError('%s takes %d arguments and the stream, got %d' % (name, n, len(args)))
        args = list(args)
        for i in pointers:
            if isinstance(args[i], torch.Tensor):
                args[i] = args[i].data_ptr()
        rc = fn(*args, self.stream)
        if rc != PSND_OK:
            check(rc, name)
    launch.__name__ = launch.__qualname__ = name
    return launch


for _name in LAUNCHABLE:
    setattr(on, _name, _launch_method(_name))


def frame_count(T, n_fft, hop, framing=FRAMING_CENTER):
    return int(lib().psnd_frame_count(int(T), int(n_fft), int(hop), int(framing)))


def build_stft_plan(n_fft, window):
    """window: array-like of n_fft taps (already centre-padded).  Returns a uint8 numpy plan."""
    w = np.ascontiguousarray(np.asarray(window, dtype=np.float32))
    if w.shape != (n_fft,):
        raise PsndError('stft plan: window must have n_fft=%d taps, got %s' % (n_fft, w.shape))
    nb = lib().psnd_stft_plan_bytes(int(n_fft))
    if nb == 0:
        raise PsndError('stft plan: n_fft=%d unsupported (power of two in [16, 8192])' % n_fft)
    plan = np.zeros(nb, dtype=np.uint8)
    check(lib().psnd_stft_plan_build(int(n_fft), np_ptr(w), np_ptr(plan)), 'psnd_stft_plan_build')
    return plan


STFT_MR_SIZES = 'even 2^a 3^b 5^c in [16, 4096]: 400, 480, 600, 800, 960, 1200, 2400, 4000 ...'


def stft_mr_covered(n_fft):
    """True where the mixed-radix STFT kernels (psnd_stft_mr_*) take this n_fft; powers of two belong to psnd_stft_*"""
    return lib().psnd_stft_mr_plan_bytes(int(n_fft)) > 0


def build_stft_mr_plan(n_fft, window):
    """plan of the mixed-radix kernels (header, window, twiddle table: include/psnd.h).  window: n_fft taps, already centre-padded."""
    w = np.ascontiguousarray(np.asarray(window, dtype=np.float32))
    if w.shape != (n_fft,):
        raise PsndError('stft plan: window must have n_fft=%d taps, got %s' % (n_fft, w.shape))
    nb = lib().psnd_stft_mr_plan_bytes(int(n_fft))
    if nb == 0:
        raise PsndError('stft plan: n_fft=%d unsupported by the mixed-radix kernels (%s)' % (n_fft, STFT_MR_SIZES))
    plan = np.zeros(nb, dtype=np.uint8)
    check(lib().psnd_stft_mr_plan_build(int(n_fft), np_ptr(w), np_ptr(plan)), 'psnd_stft_mr_plan_build')
    return plan


def build_mel_plan(mel_filter):
    W = np.ascontiguousarray(np.asarray(mel_filter, dtype=np.float32))
    M, K = W.shape
    nb = lib().psnd_mel_plan_bytes(M, K)
    plan = np.zeros(nb, dtype=np.uint8)
    check(lib().psnd_mel_plan_build(M, K, np_ptr(W), np_ptr(plan)), 'psnd_mel_plan_build')
    return plan
