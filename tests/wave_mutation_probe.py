"""Decodes the probe pictures of the reconstruction waves' BOOKKEEPING mutants with whichever build of the library
H263MI_LIB names and saves every plane.  Run as a child process by tests/test_gpu_mutation.py: a process can load one
build of the library only.

The probe pictures are small (128 x 32 and 144 x 32: one full wave per macroblock row, and a right-edge wave of one
macroblock beside it), made of the pieces of tests/wave_cases.py: macroblock row 0 holds record forms of table (a) that
carry killed coded blocks and uncoded intra blocks, macroblock row 1 a near-static wave of table (c).  Each of them shows
each of the three mutations (csrc/mutants.h).

Also here, because both sides of that test need them: the MODELS of the three mutations.  Each is exact and is obtained by
editing the RECORDS and running the oracle:
  killkeep   recon_phase_mark takes `killed` as 0                 -> the oracle over the records with kill = 0
  staticmv   recon_wave_is_static ignores any_moving              -> the oracle with the vectors zeroed in every wave the
                                                                     anatomy calls near static
  intradc    dc_nonzero taken as 0: uncoded intra blocks idle     -> the oracle with INTRADC = 0 in the uncoded blocks of
                                                                     intra macroblocks
and the anatomy says in which 8x8 blocks each may differ from the product."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "h263-rs_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import wave_cases as wc  # noqa: E402

MUTANTS = ("killkeep", "staticmv", "intradc")


def pictures():
    """four P pictures: 8 and 9 macroblocks wide, two selections of forms"""
    forms = wc._forms(False)
    killed = [f for f in forms if f[1] & f[2] and f[0] in wc.INTER_TYPES]
    killed_intra = [f for f in forms if f[1] & f[2] and f[0] in wc.INTRA_TYPES]
    uncoded_intra = [f for f in forms if f[0] in wc.INTRA_TYPES and f[1] != 63]
    out = []
    for k, mbw in enumerate((8, 9, 8, 9)):
        pick = [killed[3 * k], uncoded_intra[2 * k], killed_intra[k], killed[3 * k + 1], uncoded_intra[2 * k + 1],
                (wc.INTER, 0, 0), killed[3 * k + 2], (wc.INTER4V, 21, 0), uncoded_intra[2 * k + 8]]
        row0 = [wc._form_mb(40 * k + i, *pick[i]) for i in range(mbw)]
        v = 37 * k + 5
        row1 = wc.near_static_wave(8, v & 7, (v >> 3) & 3, (v >> 5) & 1, 1 if k & 1 else -1)
        if mbw == 9:
            row1.append(wc._form_mb(40 * k + 9, *uncoded_intra[2 * k + 9]))
        out.append(wc.picture("probe", 16 * mbw, 32, [row0, row1], wc.PICTURE_P, picture=k))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------
def mutated_records(pic, mutant):
    """the records the oracle must be given to produce what the mutant build produces"""
    mbs = wc.padded_records(pic)
    mbw, _ = wc.mb_dims(pic["w"], pic["h"])
    if mutant == "killkeep":
        mbs["kill"] = 0
    elif mutant == "staticmv":
        for a in wc.anatomy(pic):
            if a["near_static"]:
                first = a["mby"] * mbw + 8 * a["group"]
                mbs["mv"][first:first + 8] = 0
    elif mutant == "intradc":
        for i in range(len(mbs)):
            if int(mbs[i]["mb_type"]) in wc.INTRA_TYPES:
                for b in range(6):
                    if not (int(mbs[i]["cbp"]) >> b) & 1:
                        mbs[i]["intradc"][b] = 0
    else:
        raise ValueError(mutant)
    return mbs


def predicted_blocks(pic, mutant):
    """{(plane, x, y)}: the 8x8 blocks in which the mutant may differ from the product"""
    out = set()
    for a in wc.anatomy(pic):
        if mutant == "killkeep":
            tasks = a["killed_tasks"]
        elif mutant == "staticmv":
            tasks = range(wc.WAVE_TASKS) if a["near_static"] else ()
        else:
            tasks = [wc.TASK_OF[(m, b)] for m, b, dc in a["uncoded_dc"] if dc != 0]
        out |= {wc.task_region(t, a["mby"], a["group"]) for t in tasks}
    return out


def reference(pic):
    from oracle import oracle as orc
    mbs, co = wc.reference_records(pic["w"], pic["h"])
    rc, ref = orc.decode_picture(pic["w"], pic["h"], mbs, co, None)
    assert rc == 0
    return ref


def expectations(mutant=None):
    """[(name, picture, planes)]: the oracle's planes, or with a mutant's name its model's"""
    from oracle import oracle as orc
    out = []
    for k, pic in enumerate(pictures()):
        mbs = mutated_records(pic, mutant) if mutant else pic["mbs"]
        rc, want = orc.decode_picture(pic["w"], pic["h"], mbs, pic["coeffs"], reference(pic))
        assert rc == 0
        out.append(("p%d" % k, pic, want))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the child: decode everything with the library under test, through k_recon and through k_frame
# ---------------------------------------------------------------------------------------------------------------
def decode_all():
    import h263mi
    import test_gpu_wave_sweep as gpu                            # (its batch runner: key frame, then the picture, in a pipelined batch)
    out = {}
    st = h263mi.H263State()
    for k, pic in enumerate(pictures()):
        w, h = pic["w"], pic["h"]
        mbs, co = wc.reference_records(w, h)
        st.submit_picture(w, h, mbs, co, h263mi.PICTURE_I)
        st.submit_picture(w, h, pic["mbs"], pic["coeffs"], h263mi.PICTURE_P, temporal_reference=1)
        out["state_p%d" % k] = st.get_last_picture().as_yuv()
        out["frame_p%d" % k] = gpu.decode_batch([(pic, None)], 8, "dense", "probe picture %d" % k)[0]
    st.close()
    return out


if __name__ == "__main__":
    res = decode_all()
    np.savez(sys.argv[1], **{"%s_%d" % (name, i): p for name, planes in res.items() for i, p in enumerate(planes)})
