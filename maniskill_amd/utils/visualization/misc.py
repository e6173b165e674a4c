"""Picture helpers of `render()` and the episode videos (counterpart of mani_skill/utils/visualization/misc.py:
`tile_images` with the reference's tiling rule, `images_to_video`).

Videos are written as mp4 through imageio where it imports; otherwise as an animated PNG through PIL, a format every
browser plays. Where neither imports, `images_to_video` raises an ImportError that says so.
"""
import os
from typing import List, Sequence

import numpy as np
import torch


def tile_images(images: Sequence, nrows: int = 1):
    """One picture of several, laid out in columns from left to right; numpy arrays or torch tensors, [H, W, 3] or
    batched [B, H, W, 3] (one batch size for all). The canvas is `nrows` times the first picture's height tall. With
    nrows == 1 the pictures are first ordered by falling height (a stable sort) and may differ in size; a picture joins the
    current column while the column stays within the canvas height and the picture is as wide as the column, otherwise
    it starts the next column. What the pictures leave uncovered is zero."""
    images = list(images)
    h_ax = 1 if images[0].ndim == 4 else 0
    if nrows == 1:
        images = sorted(images, key=lambda im: im.shape[h_ax], reverse=True)
    canvas_h = images[0].shape[h_ax] * nrows
    columns, used, width = [[]], 0, images[0].shape[h_ax + 1]
    for im in images:
        h, w = im.shape[h_ax], im.shape[h_ax + 1]
        if columns[-1] and not (used + h <= canvas_h and w == width):
            columns.append([])
            used, width = 0, w
        columns[-1].append(im)
        used += h
    shape = tuple(images[0].shape[:h_ax]) + (canvas_h, sum(c[0].shape[h_ax + 1] for c in columns), 3)
    first = images[0]
    out = first.new_zeros(shape) if isinstance(first, torch.Tensor) else np.zeros(shape, dtype=first.dtype)
    x = 0
    for column in columns:
        y, w = 0, column[0].shape[h_ax + 1]
        for im in column:
            h = im.shape[h_ax]
            out[..., y : y + h, x : x + w, :] = im
            y += h
        x += w
    return out


def _writers():
    """(imageio or None, PIL.Image or None)"""
    try:
        import imageio
    except ImportError:
        imageio = None
    try:
        from PIL import Image
    except ImportError:
        Image = None
    return imageio, Image


def video_backend() -> str:
    """"imageio" (mp4), "pil" (animated PNG), or an ImportError naming both"""
    imageio, Image = _writers()
    if imageio is not None:
        return "imageio"
    if Image is not None:
        return "pil"
    raise ImportError("writing a video needs imageio (mp4) or PIL (an animated PNG); neither can be imported")


def images_to_video(images: List, output_dir: str, video_name: str, fps: int = 10, quality: float = 5, verbose: bool = True, **kwargs) -> str:
    """Writes the frames (uint8 [H, W, 3] each, RGB) as one video file in `output_dir` and returns its path:
    <video_name>.mp4 through imageio, else <video_name>.png, an animated PNG, through PIL."""
    backend = video_backend()
    frames = [np.ascontiguousarray(im.cpu().numpy() if isinstance(im, torch.Tensor) else im, dtype=np.uint8) for im in images]
    assert frames and all(f.ndim == 3 and f.shape == frames[0].shape for f in frames), "a video is a list of equally sized [H, W, 3] frames"
    os.makedirs(output_dir, exist_ok=True)
    stem = os.path.join(output_dir, video_name.replace(" ", "_").replace("\n", "_"))
    if backend == "imageio":
        imageio, _ = _writers()
        path = stem + ".mp4"
        writer = imageio.get_writer(path, fps=fps, quality=quality, **kwargs)
        for f in frames:
            writer.append_data(f)
        writer.close()
    else:
        _, Image = _writers()
        path = stem + ".png"
        pics = [Image.fromarray(f) for f in frames]
        # (default_image=False: frame 0 is part of the animation; each frame is shown for 1000 / fps milliseconds)
        pics[0].save(path, format="PNG", save_all=True, append_images=pics[1:], duration=1000.0 / fps, loop=0)
    if verbose:
        print(f"Video created: {path}")
    return path
