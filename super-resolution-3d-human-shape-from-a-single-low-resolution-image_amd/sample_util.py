"""The point-cloud dumps of the reference's training loop (lib/sample_util.py): ASCII PLY files of coloured vertices, byte for byte
the reference's - six decimals per coordinate, integer colours, '\\n' line ends - so that a viewer or a script written for its files
reads these."""
import numpy as np

_HEADER = ("ply", "format ascii 1.0", "element vertex %d", "property float x", "property float y", "property float z",
           "property uchar red", "property uchar green", "property uchar blue", "end_header")


def _write_ply(fname, points, colours):
    """points [N,3], colours [N,3] (written with %d: truncated towards zero, as the reference's formatter does)."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    colours = np.asarray(colours, np.float64).reshape(-1, 3)
    if len(points) != len(colours):
        raise ValueError("%d points against %d colours" % (len(points), len(colours)))
    with open(fname, "w", newline="\n") as f:
        f.write("\n".join(_HEADER) % len(points) + "\n")
        for (x, y, z), (r, g, b) in zip(points, colours):
            f.write("%.6f %.6f %.6f %d %d %d\n" % (x, y, z, r, g, b))


def save_samples_truncted_prob(fname, points, prob):
    """points [N,3], prob [N,1] (or [N]) in 0..1: red where prob > 0.5, green where prob < 0.5, black at exactly 0.5."""
    prob = np.asarray(prob).reshape(-1, 1)
    _write_ply(fname, points, np.concatenate([(prob > 0.5) * 255, (prob < 0.5) * 255, np.zeros(prob.shape)], -1))


def save_samples_rgb(fname, points, rgb):
    """points [N,3], rgb [N,3] in 0..1, written as 255 rgb."""
    _write_ply(fname, points, np.asarray(rgb) * 255)
