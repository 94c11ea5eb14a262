from .synth import SynthOCT    # noqa: F401
from .npz import NpzOCT        # noqa: F401


def EyeSetGenerator(dbname='synth', **kw):
    """reference data/octgen.py:35 entry point.  `synth` / `goals`: the synthetic GOALS-shaped generator (5 classes).  `npz:PATH`: stored
    B-scans packed by tools/pack_dataset.py, kept on the device and augmented there (data/npz.py; `crop=(H, W)` is the reference's
    make_tran(256, 256)).  Image decoding and the cv2 / albumentations loader itself stay out of scope."""
    if dbname in ('synth', 'goals'):
        return SynthOCT(dbname=dbname, **kw)
    if dbname.startswith('npz:'):
        return NpzOCT(dbname[4:], **kw)
    raise ValueError(f"--db={dbname!r}: available are 'synth'/'goals' (synthetic 5-class 800x1100 B-scans) and 'npz:PATH' (a file packed by tools/pack_dataset.py)")
