#!/usr/bin/env python3
"""Generates tests/golden/envlight_cases.npz from the REFERENCE'S OWN InfiniteAreaLight compiled in place (oracle/ref_hotpath.cpp ->
oracle/_ref/libref_hotpath.so, `make -C oracle ref`): Le, Pdf_Li and Sample_Li on the ten maps of tests/envlight_cases.py, and
PathTracer::Li on its two scenes.  The reference exists only in the build container, so this script runs there only:

    python tests/golden/make_envlight_golden.py        (rewrites tests/golden/envlight_cases.npz; commit the result)

The fixture is data only: per map its SHA-256 and the sin(theta) row weights the cases are built from, what the reference returned for
the cases, and for the Li scenes the camera rays the reference made and what Li returned for them.  The calls run with correctly
rounded trigonometry (what the kernels compute), the constructor with the C library's, as in make_refpin_golden.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import envlight_cases as ec  # noqa: E402
from make_refpin_golden import save  # noqa: E402

NAME = "envlight_cases.npz"


def load():
    return np.load(os.path.join(HERE, NAME))


def map_answers(s, light, name, weights):
    """what the reference's light `light` of scene s returns for the cases of map `name`"""
    u, _ = ec.draws(name, weights)
    d = ec.directions(name)
    wi, pdf, le, ok = s.env_sample_li(light, u)
    return dict(wi=wi, pdf=pdf, sle=le, ok=ok.astype(np.int32), le=s.env_le(light, d), pdf_li=s.env_pdf_li(light, d))


def generate():
    """-> {array name: array} from the reference harness"""
    from oracle import ref_binding as rb
    out = {}
    for name in ec.MAPS:
        h = ec.map_size(name)[1]
        out["sha256/" + name] = np.frombuffer(bytes.fromhex(ec.map_sha256(name)), "<i4")
        out["weights/%d" % h] = ec.oracle_row_weights(h)
    try:
        for name in ec.MAPS:
            rb.set_trig_mode(rb.TRIG_LIBM)       # the constructor's sin(theta) weights are host-side
            s = ec.map_scene(name).instantiate(rb.RefScene())
            rb.set_trig_mode(rb.TRIG_CORRECTLY_ROUNDED)
            for key, a in map_answers(s, 0, name, out["weights/%d" % ec.map_size(name)[1]]).items():
                out["%s/%s" % (name, key)] = a
        for k, name in enumerate(ec.LI_SCENES):
            rb.set_trig_mode(rb.TRIG_LIBM)
            s = ec.li_scene(name).instantiate(rb.RefScene())
            st, states = ec.li_film_inputs(k)
            rays, start = s.camera_rays(st, states)
            rb.set_trig_mode(rb.TRIG_CORRECTLY_ROUNDED)
            L, after, draws, calls = s.li(rays, start, ec.LI_DEPTH)
            out.update({"li_%s/rays" % name: rays, "li_%s/states" % name: start, "li_%s/L" % name: L, "li_%s/after" % name: after,
                        "li_%s/draws" % name: draws.astype(np.int32), "li_%s/calls" % name: np.array(calls, np.int32)})
            if name == "two_maps":      # each map of the two-map scene answers as it does alone
                for light, m in enumerate(ec.TWO_MAPS):
                    if m is None:
                        continue
                    for key, a in map_answers(s, light, m, out["weights/%d" % ec.map_size(m)[1]]).items():
                        assert a.tobytes() == out["%s/%s" % (m, key)].tobytes(), (m, key)
    finally:
        rb.set_trig_mode(rb.TRIG_LIBM)
    return out


def main():
    save(NAME, generate())
    print(NAME, os.path.getsize(os.path.join(HERE, NAME)))


if __name__ == "__main__":
    main()
