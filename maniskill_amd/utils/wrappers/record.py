"""RecordEpisode: trajectory recording in the reference's container layout, and episode videos of `env.render()`
frames (counterpart of mani_skill/utils/wrappers/record.py:195-760).

On disk, next to each other:
  <name>.json   env_info {env_id, max_episode_steps, env_kwargs}, source_type / source_desc, and per
                trajectory an entry of `episodes`: episode_id, episode_seed, control_mode,
                elapsed_steps, reset_kwargs, success / fail of the last frame  (record.py:663-728)
  <name>.h5     groups traj_<id> with datasets obs [T+1,...], actions [T,A], terminated [T],
                truncated [T], success / fail [T], rewards [T], env_states/{actors,articulations}/<name>
                [T+1, D]                                                     (record.py:594-726)
h5py is not part of this image: without it the same tree is written as <name>.npz with the dataset
paths as keys ("traj_0/env_states/actors/cube", ...). `maniskill_amd.trajectory.utils.load_h5_data`
reads either.

With `save_video=True` every reset and step adds one `env.render()` frame (all envs tiled into one picture); a video is
written at the next full reset, at `flush_video()` / `close()`, or whenever it holds `max_steps_per_video` steps:
<output_dir>/<video id>.mp4 through imageio, or .png (animated) through PIL where imageio is missing
(maniskill_amd/utils/visualization/misc.py). The frames are the flat-shaded view of this build, so the env needs a
working `render_mode` ("rgb_array", "sensors" or "all").
"""
import json
import os
from typing import Optional

import numpy as np
import torch

import gymnasium as gym

from maniskill_amd.utils import common

try:  # pragma: no cover - not installed in this image
    import h5py
except ImportError:
    h5py = None


def parse_env_info(env):
    base = env.unwrapped
    spec = getattr(base, "spec", None) or getattr(env, "spec", None)
    if spec is None:
        return None
    return dict(env_id=spec.id, max_episode_steps=getattr(spec, "max_episode_steps", None), env_kwargs=_jsonable(dict(getattr(spec, "kwargs", {}) or {})))


def _jsonable(x):
    if isinstance(x, dict):
        return {str(k): _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().tolist()
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (np.integer,)):
        return int(x)
    if isinstance(x, (np.floating,)):
        return float(x)
    if isinstance(x, (np.bool_,)):
        return bool(x)
    if isinstance(x, (str, int, float, bool)) or x is None:
        return x
    return str(x)


def _np(x):
    if isinstance(x, dict):
        return {k: _np(v) for k, v in x.items()}
    return common.to_numpy(x)


class RecordEpisode(gym.Wrapper):
    def __init__(self, env, output_dir: str, save_trajectory: bool = True, trajectory_name: Optional[str] = None, save_on_reset: bool = True,
                 record_reward: bool = True, record_env_state: bool = True, source_type: Optional[str] = None, source_desc: Optional[str] = None,
                 save_video: bool = False, info_on_video: bool = False, video_fps: int = 30, max_steps_per_video: Optional[int] = None, **_unused):
        super().__init__(env)
        self.save_video = save_video
        self.video_fps, self.max_steps_per_video = video_fps, max_steps_per_video
        self._video_frames, self._video_id, self._video_steps = [], -1, 0
        if save_video:
            from maniskill_amd.utils.visualization.misc import video_backend

            if info_on_video:
                raise NotImplementedError("info_on_video draws text on the frames, which this build does not do")
            mode = getattr(env.unwrapped, "render_mode", None)
            if mode not in ("rgb_array", "sensors", "all"):
                raise ValueError(f"save_video=True records env.render() frames: make the env with render_mode=\"rgb_array\", \"sensors\" or \"all\" (it has {mode!r})")
            video_backend()  # (an ImportError here, not after an episode, where neither imageio nor PIL imports)
        self.output_dir = output_dir
        os.makedirs(output_dir, exist_ok=True)
        self.save_trajectory = save_trajectory
        self.save_on_reset = save_on_reset
        self.record_reward = record_reward
        self.record_env_state = record_env_state
        self._name = trajectory_name or "trajectory"
        self._json_path = os.path.join(output_dir, self._name + ".json")
        self._data_path = os.path.join(output_dir, self._name + (".h5" if h5py is not None else ".npz"))
        self._json_data = dict(env_info=parse_env_info(env), episodes=[])
        if source_type is not None:
            self._json_data["source_type"] = source_type
        if source_desc is not None:
            self._json_data["source_desc"] = source_desc
        self._datasets = {}  # "traj_i/..." -> array
        self._episode_id = -1
        self._frames = None
        self.last_reset_kwargs = {}

    @property
    def base_env(self):
        return self.env.unwrapped

    @property
    def num_envs(self):
        return self.base_env.num_envs

    # ------------------------------------------------------------------ buffers
    def _new_buffers(self):
        self._frames = dict(obs=[], state=[], action=[], reward=[], terminated=[], truncated=[], success=[], fail=[])
        self._ptr = np.zeros(self.num_envs, dtype=np.int64)  # first frame of the running episode of each env

    def _push(self, obs, action, reward, terminated, truncated, info):
        f = self._frames
        f["obs"].append(_np(obs))
        if self.record_env_state:
            f["state"].append(_np(self.base_env.get_state_dict()))
        f["action"].append(action)
        f["reward"].append(reward)
        f["terminated"].append(terminated)
        f["truncated"].append(truncated)
        f["success"].append(_np(info["success"]).astype(bool) if info is not None and "success" in info else None)
        f["fail"].append(_np(info["fail"]).astype(bool) if info is not None and "fail" in info else None)

    # ------------------------------------------------------------------ video
    def capture_image(self) -> np.ndarray:
        """uint8 [H', W', 3]: env.render() with the envs tiled into one picture (a near-square grid)"""
        from maniskill_amd.utils.visualization.misc import tile_images

        frames = common.to_numpy(self.env.render())
        if frames.ndim == 3:
            return frames
        rows = int(np.sqrt(len(frames)))
        return tile_images(list(frames), nrows=rows) if len(frames) > 1 else frames[0]

    def flush_video(self, name: Optional[str] = None, verbose: bool = False, save: bool = True):
        """writes the collected frames as one video (nothing without frames) and starts the next"""
        from maniskill_amd.utils.visualization.misc import images_to_video

        path = None
        if save and len(self._video_frames) > 1:
            self._video_id += 1
            path = images_to_video(self._video_frames, self.output_dir, name if name is not None else str(self._video_id), fps=self.video_fps, verbose=verbose)
        self._video_frames, self._video_steps = [], 0
        return path

    # ------------------------------------------------------------------ gym API
    def reset(self, *args, seed=None, options=None, **kwargs):
        if self.save_video and self.save_on_reset and (options is None or "env_idx" not in options):
            self.flush_video()
        if self.save_on_reset and self.save_trajectory and self._frames is not None:
            idx = None
            if options is not None and "env_idx" in options:
                idx = common.to_numpy(options["env_idx"])
            self.flush_trajectory(env_idxs_to_flush=idx)
        obs, info = super().reset(*args, seed=seed, options=options, **kwargs)
        self.last_reset_kwargs = _jsonable(dict(seed=seed, options=options if options is None or "env_idx" not in options else None))
        if self._frames is None or options is None or "env_idx" not in (options or {}):
            self._new_buffers()
        N = self.num_envs
        adim = self.base_env.single_action_space.shape[0]
        self._push(obs, np.zeros((N, adim), np.float32), np.zeros(N, np.float32), np.zeros(N, bool), np.zeros(N, bool), None)
        if options is not None and "env_idx" in options:
            self._ptr[common.to_numpy(options["env_idx"])] = len(self._frames["obs"]) - 1
        if self.save_video:
            self._video_frames.append(self.capture_image())
        return obs, info

    def step(self, action):
        obs, rew, terminated, truncated, info = super().step(action)
        N = self.num_envs
        self._push(obs, _np(action).reshape(N, -1).astype(np.float32), _np(rew).reshape(N).astype(np.float32),
                   _np(terminated).reshape(N).astype(bool), np.broadcast_to(_np(truncated), (N,)).astype(bool), info)
        if self.save_video:
            self._video_frames.append(self.capture_image())
            self._video_steps += 1
            if self.max_steps_per_video is not None and self._video_steps >= self.max_steps_per_video:
                self.flush_video()
        return obs, rew, terminated, truncated, info

    # ------------------------------------------------------------------ flushing
    def flush_trajectory(self, verbose=False, ignore_empty_transition=True, env_idxs_to_flush=None, save=True):
        if self._frames is None:
            return
        f = self._frames
        end = len(f["obs"])
        idxs = np.arange(self.num_envs) if env_idxs_to_flush is None else np.asarray(env_idxs_to_flush)

        def sl(frames, start, e):
            first = frames[start]
            if isinstance(first, dict):
                return {k: sl([fr[k] for fr in frames], start, e) for k in first}
            return np.stack([fr[e] for fr in frames[start:end]])

        for e in idxs:
            start = int(self._ptr[e])
            if ignore_empty_transition and end - start <= 1:
                continue
            if save:
                self._episode_id += 1
                g = f"traj_{self._episode_id}"
                self._put(g + "/obs", sl(f["obs"], start, e))
                self._put(g + "/actions", np.stack([a[e] for a in f["action"][start + 1 : end]]).astype(np.float32))
                self._put(g + "/terminated", np.array([t[e] for t in f["terminated"][start + 1 : end]], dtype=bool))
                self._put(g + "/truncated", np.array([t[e] for t in f["truncated"][start + 1 : end]], dtype=bool))
                info = dict(episode_id=self._episode_id, episode_seed=int(np.asarray(self.base_env._episode_seed).reshape(-1)[e]),
                            control_mode=self.base_env.control_mode, elapsed_steps=end - start - 1,
                            reset_kwargs=self.last_reset_kwargs if self.num_envs == 1 else dict())
                for key in ("success", "fail"):
                    vals = f[key][start + 1 : end]
                    if len(vals) and vals[0] is not None:
                        arr = np.array([v[e] for v in vals], dtype=bool)
                        self._put(g + "/" + key, arr)
                        info[key] = bool(arr[-1])
                if self.record_env_state:
                    self._put(g + "/env_states", sl(f["state"], start, e))
                if self.record_reward:
                    self._put(g + "/rewards", np.array([r[e] for r in f["reward"][start + 1 : end]], dtype=np.float32))
                self._json_data["episodes"].append(info)
                if verbose:
                    print(f"Recorded episode {self._episode_id}")
        self._ptr[idxs] = end - 1
        if save:
            self._write()

    def _put(self, key, value):
        if isinstance(value, dict):
            for k, v in value.items():
                self._put(key + "/" + k, v)
        else:
            self._datasets[key] = np.asarray(value)

    def _write(self):
        with open(self._json_path, "w") as fh:
            json.dump(_jsonable(self._json_data), fh, indent=2)
        if h5py is not None:  # pragma: no cover
            with h5py.File(self._data_path, "w") as h5:
                for k, v in self._datasets.items():
                    h5.create_dataset(k, data=v)
        else:
            np.savez_compressed(self._data_path, **self._datasets)

    def close(self):
        if self.save_trajectory and self._frames is not None:
            self.flush_trajectory()
        if self.save_video:
            self.flush_video()
        return super().close()
