"""Writes tests/golden/plot_scene.npz: what matplotlib and the reference say about the scene of `utils/plot_script.py:plot_3d_motion`, for
tests/test_plot_host.py.  Runs on a development machine with matplotlib and a checkout of the reference; nothing else imports matplotlib.

    python tests/golden/make_plot_golden.py /path/to/reference

  points (64, 3)              world points: the corners of the axes box, a grid on the ground, the joints of a pose
  pixels_1000, pixels_64      (64, 2) fp64 (col, row), row 0 on top, where matplotlib puts them in a 10 x 10 inch figure of that many pixels a side
                              with the reference's settings (limits, view_init(120, -90), dist 5.5, axis off)
  colour_names, colour_rgb    the named colours of the reference's list and of the trajectory, as matplotlib resolves them
  chain_colours               the reference's colour list, as indices into colour_names
  smpl_chain_*, smplx_chain_* the two kinematic chain lists as recorded from the reference: joints flat, and the length of each chain
  matplotlib_version"""
import os
import sys

import numpy as np


def main(reference_root):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.colors as mcolors
    import matplotlib.pyplot as plt
    from mpl_toolkits.mplot3d import proj3d

    sys.path.insert(0, reference_root)
    from utils import plot_script

    radius = 4
    rng = np.random.default_rng(26)
    box = np.asarray([(x, y, z) for x in (-radius / 2, radius / 2) for y in (0, radius) for z in (0, radius)], dtype=np.float64)
    ground = np.asarray([(x, 0.0, z) for x in np.linspace(-3.0, 3.0, 4) for z in np.linspace(-2.5, 5.0, 4)])
    pose = np.concatenate([rng.uniform(-0.6, 0.6, (40, 1)), rng.uniform(0.0, 1.8, (40, 1)), rng.uniform(-0.6, 0.6, (40, 1))], 1)
    points = np.concatenate([box, ground, pose])
    out = {"points": points, "matplotlib_version": np.asarray(matplotlib.__version__)}
    for size in (1000, 64):
        fig = plt.figure(figsize=(10, 10), dpi=size / 10)
        ax = fig.add_subplot(111, projection="3d")
        ax.view_init(elev=120, azim=-90)
        ax._dist = 5.5                      # `ax.dist = 5.5` in the reference: the attribute matplotlib 3.10 reads
        ax.set_xlim3d([-radius / 2, radius / 2])
        ax.set_ylim3d([0, radius])
        ax.set_zlim3d([0, radius])
        plt.axis("off")
        fig.canvas.draw()
        assert fig.canvas.get_width_height() == (size, size)
        x, y, _ = proj3d.proj_transform(points[:, 0], points[:, 1], points[:, 2], ax.get_proj())
        disp = ax.transData.transform(np.stack([x, y], 1))
        out[f"pixels_{size}"] = np.stack([disp[:, 0], size - disp[:, 1]], 1)
        plt.close(fig)
    colours = ["red", "blue", "black", "red", "blue"] + ["darkblue"] * 5 + ["darkred"] * 5      # plot_script.py:121-123
    names = sorted(set(colours))
    out["colour_names"] = np.asarray(names)
    out["colour_rgb"] = np.asarray([mcolors.to_rgb(n) for n in names], dtype=np.float64)
    out["chain_colours"] = np.asarray([names.index(c) for c in colours], dtype=np.int32)
    for key, chains in (("smpl", plot_script.smpl_kinematic_chain), ("smplx", plot_script.smplx_kinematic_chain)):
        out[f"{key}_chain_joints"] = np.asarray([j for c in chains for j in c], dtype=np.int32)
        out[f"{key}_chain_lengths"] = np.asarray([len(c) for c in chains], dtype=np.int32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plot_scene.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {len(points)} points, origin-like first pixel {out['pixels_1000'][0]}")


if __name__ == "__main__":
    main(sys.argv[1])
