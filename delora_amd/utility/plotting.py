"""The six-row figure of a logged step (what the reference draws with cv2 + pyplot in src/utility/plotting.py:12-58), drawn with
matplotlib alone on an Agg canvas of its own (the process-wide backend is left as it is).  matplotlib is an optional dependency: it is imported inside the function, so that runs
which log no images never need it."""
import numpy as np

SUBTITLES = ("Target image at time t",
             "Source at time t+1",
             "Network transformed source image at time t+1",
             "Po2Pl loss (on transformed source points)",
             "Normal map of target",
             "Normal map of transformed source")
SUBTITLE_SOURCE_TRAINING = "Randomly transformed Source at time t+1"


def _as_image(t):
    """``[1,C,H,W]`` tensor or array -> float ``[3,H,W]`` numpy array with the columns flipped (azimuth grows to the left)."""
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.asarray(a[0][:3], dtype=np.float64)[:, :, ::-1]


def row_colours(image, as_normals, turbo):
    """uint8 ``[H,W,3]`` of one row: the turbo-coloured norm of the three channels scaled to its maximum (rows 0-3), or (n + 1) / 2
    scaled to its maximum as RGB (rows 4-5); pixels whose three channels are all zero are black.  Returns (colours, norm)."""
    norm = np.sqrt(image[0] ** 2 + image[1] ** 2 + image[2] ** 2)
    if as_normals:
        half = (image + 1.0) / 2.0
        top = float(np.max(half)) if half.size else 0.0
        rgb = np.moveaxis(half, 0, -1) * (255.0 / top if top > 0 else 0.0)
    else:
        top = float(np.max(norm)) if norm.size else 0.0
        level = (norm * (255.0 / top if top > 0 and np.isfinite(top) else 0.0))
        rgb = turbo(np.nan_to_num(level).astype(np.uint8))[..., :3] * 255.0
    rgb = np.nan_to_num(rgb).astype(np.uint8)
    rgb[norm == 0] = 0
    return rgb, norm


def plot_lidar_image(input, label, iteration, path, training):
    """Write the figure of six images (each ``[1,>=3,H,W]``) to ``path`` (PNG) and return ``path``."""
    try:
        import matplotlib
        from matplotlib.figure import Figure
        from matplotlib.backends.backend_agg import FigureCanvasAgg
    except ImportError as e:                                          # pragma: no cover
        raise RuntimeError("drawing the logged images needs matplotlib, which is not installed: install it, or switch the "
                           "config key `visualize_images` off") from e
    turbo = matplotlib.colormaps["turbo"]
    fig = Figure(figsize=(6.4, 4.8))
    FigureCanvasAgg(fig)
    axes = fig.subplots(len(input), 1, gridspec_kw={"wspace": 0, "hspace": 0})
    fig.suptitle("Results at iteration " + str(iteration))
    for index, ax in enumerate(np.atleast_1d(axes)):
        rgb, norm = row_colours(_as_image(input[index]), index >= 4, turbo)
        scale = ax.imshow(norm, cmap="turbo")                         # the colour bar's scale: the norm itself
        ax.imshow(rgb, aspect=max(1, 4 - int(rgb.shape[0] / 32)))
        ax.grid(True, linewidth=0.5, alpha=0.5)
        ax.set_xticklabels([])
        ax.set_yticklabels([])
        title = SUBTITLE_SOURCE_TRAINING if (index == 1 and training) else SUBTITLES[index % len(SUBTITLES)]
        ax.text(1.0, 0.01, title, verticalalignment="bottom", horizontalalignment="right", transform=ax.transAxes, color="w").set_alpha(.6)
        fig.colorbar(scale, ax=ax)
    fig.savefig(path)
    return path
