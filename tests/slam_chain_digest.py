"""Child process of tests/test_gpu_slam_chunk.py: a short TrackSIM run whose frames carry several SLAM chunks,
printed as one line "digest <sha256> slam <feature updates> frames <n>".  The digest covers every frame's state
vector and layout and the final first-estimate vector and covariance, byte for byte, so two runs compare the SLAM
chunk's two launch chains (UVIO_HP_SLAM_SEVEN in the environment selects the seven-launch one) bit for bit.

usage: python tests/slam_chain_digest.py [FRAMES]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import uvio_amd as U  # noqa: E402
from uvio_amd.sim import SimStream  # noqa: E402


def main():
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    cfg = os.path.join(ROOT, "configs", "euroc_mav", "estimator_config.yaml")
    opts = U.load_options(cfg, max_msckf_in_update=60, max_slam_features=10, max_slam_in_update=4, dt_slam_delay=0.3)
    sim = SimStream(opts, duration=n_frames / opts.track_frequency + 1.2, seed=7, spawn=60, frac_long=0.3)
    g = U.VioManager(opts, device=0)
    h = hashlib.sha256()
    count = {"slam": 0}

    def after(nf, t):
        x, meta = g.get_state_vector()
        h.update(x.tobytes())
        h.update(meta.tobytes())
        count["slam"] += g.get_timing()["n_slam"]

    sim.run(g, n_frames=n_frames, on_frame=after)
    h.update(g.get_fej_vector().tobytes())
    h.update(np.ascontiguousarray(g.get_cov()).tobytes())
    g.close()
    print("digest %s slam %d frames %d" % (h.hexdigest(), count["slam"], n_frames))


if __name__ == "__main__":
    main()
