#!/usr/bin/env python
"""Generate tests/golden/utils_sound.npz by IMPORTING the reference's pytorch_sound/utils/sound.py (read-only; its location: PSND_REFERENCE,
as tools/gen_golden.py) and running its two scipy filters.

The packages that module imports at its top and this image lacks (pretty_midi, pyworld, pysndfx, librosa) are stubbed by `install_stubs()`
of tools/gen_golden.py; none of them is called here.  The fixture is data only: a seeded (2, 4099) float32 input and the reference's
`preemphasis` / `inv_preemphasis` of it at coeff 0.97 and 0.5.  `lowpass` is not in it: the reference pipes it through sox, which cannot
run here (pytorch_sound_amd/utils/sound.py).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402  (puts the repository and the reference on sys.path)


def main():
    gen_golden.install_stubs()
    from pytorch_sound.utils import sound as ref
    assert os.path.abspath(ref.__file__).startswith(os.path.abspath(gen_golden.REF)), ref.__file__
    x = gen_golden.seeded_wav(31, 2, 4099)
    out = {'x': x}
    for coeff in (0.97, 0.5):
        tag = ('%g' % coeff).replace('.', 'p')
        out['preemphasis_' + tag] = ref.preemphasis(x, coeff)
        out['inv_preemphasis_' + tag] = ref.inv_preemphasis(x, coeff)
    for k, v in out.items():
        assert v.dtype == np.float32 and v.shape == x.shape, (k, v.dtype, v.shape)
    path = os.path.join(gen_golden.OUT, 'utils_sound.npz')
    np.savez(path, **out)
    print('wrote', path, {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
