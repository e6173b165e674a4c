from .misc import images_to_video, tile_images  # noqa: F401
