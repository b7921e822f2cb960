"""Decodes the designed tables of tests/idct_form_cases.py with whichever build of the library H263MI_LIB names, through
k_recon (H263State) and through k_frame (a frame-pipelined batch of 8), and saves every plane.  Run as a child process by
tests/test_gpu_mutation.py: a process can load one build of the library only.

The pictures put the blocks of the two mutation fixtures (tests/golden/idct_sensitive_blocks.json, idct_sensitive_forms.json)
through every form a reconstruction round is compiled in; which round is which form is the declaration of idct_form_cases, and
what a mutation makes of a listed block is the fixture's soft-float prediction."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "h263-rs_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import idct_form_cases as fc  # noqa: E402

PATHS = ("state", "frame")


def pictures():
    """[(name, picture)] in the order of the tables"""
    return [("%s%d" % (name, i), pic) for name, i, pic in fc.all_pictures()]


def expectations():
    """[(name, picture, the oracle's planes)]"""
    from oracle import oracle as orc
    out = []
    for name, pic in pictures():
        rc, want = orc.decode_picture(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], fc.flat_reference()[2] if pic["base"] else None)
        assert rc == 0
        out.append((name, pic, want))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the child: decode everything with the library under test
# ---------------------------------------------------------------------------------------------------------------
def decode_all():
    import h263mi
    import test_gpu_wave_sweep as gpu                            # (its batch runner: key frame, then the pictures, in a pipelined batch)
    gpu.reference = fc.flat_reference                            # (this process decodes nothing else)
    out = {}
    pics = pictures()
    key_mbs, key_co, _ = fc.flat_reference()
    st = h263mi.H263State()
    for name, pic in pics:
        if pic["base"]:
            st.submit_picture(pic["w"], pic["h"], key_mbs, key_co, h263mi.PICTURE_I)
        st.submit_picture(pic["w"], pic["h"], pic["mbs"], pic["coeffs"], pic["picture_type"], temporal_reference=1)
        out["state_" + name] = st.get_last_picture().as_yuv()
    st.close()
    for run in gpu.groups_by_size([(pic, name) for name, pic in pics]):
        for (_, name), planes in zip(run, gpu.decode_batch(run, 8, "dense", "form probe")):
            out["frame_" + name] = planes
    return out


if __name__ == "__main__":
    res = decode_all()
    np.savez(sys.argv[1], **{"%s_%d" % (name, i): p for name, planes in res.items() for i, p in enumerate(planes)})
