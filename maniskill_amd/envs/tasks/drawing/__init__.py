"""the reference keeps its drawing tasks in a package of their own: the same import path, the class of tasks/tabletop/draw_triangle.py"""
from maniskill_amd.envs.tasks.tabletop.draw_triangle import DrawTriangleEnv  # noqa: F401
