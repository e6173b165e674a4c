"""env-steps/s with the ray-cast camera observations beside the state observations, and the ray-cast launch's mean time by
device events: `--env-id` (PickCube-v1) at `--num-envs` (1024) envs with `--obs-mode` (depth+segmentation), the cameras at
`--size` (128) pixels square, random actions, `--runs` (3) runs of `--steps` (200) steps after `--warmup` (20) steps without a
reset in between, in one process; then the same loop with obs_mode="state". One JSON line per mode, then both as RESULT.
`--camera` keeps one of the env's cameras (e.g. fetch_head of SceneManipulation-v1's Fetch) and drops the others before the
first step; `--robot-uids` picks the robot of an env that offers several. `--shade` also times the shading launch of the
flat-shaded view (`Camera.capture_picture`) with the same device-event loop, beside the depth launch of the same process."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import maniskill_amd.envs  # noqa: F401  (installs the gymnasium stand-in where the package is absent)
import gymnasium as gym

ap = argparse.ArgumentParser()
ap.add_argument("--env-id", default="PickCube-v1")
ap.add_argument("--num-envs", type=int, default=1024)
ap.add_argument("--obs-mode", default="depth+segmentation")
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--camera", default=None, help="render this camera only (default: every camera the env declares)")
ap.add_argument("--robot-uids", default=None, help="the env's robot (default: the env's own default)")
ap.add_argument("--shade", action="store_true", help="time the shading launch (capture_picture) beside the depth launch")
args = ap.parse_args()
N, STEPS, WARMUP, RUNS = args.num_envs, args.steps, args.warmup, args.runs

out = {}
for mode in (args.obs_mode, "state"):
    robot = dict(robot_uids=args.robot_uids) if args.robot_uids is not None else {}
    env = gym.make(args.env_id, num_envs=N, obs_mode=mode, sensor_configs=dict(width=args.size, height=args.size), **robot).unwrapped
    if args.camera is not None:
        for uid in [u for u in env._sensors if u != args.camera]:
            del env._sensors[uid]
        assert list(env._sensors) == [args.camera], f"{args.env_id} has no camera {args.camera!r}"
    env.reset(seed=0)
    g = torch.Generator(device=env.device).manual_seed(1)
    actions = [2 * torch.rand(N, *env.single_action_space.shape, device=env.device, generator=g) - 1 for _ in range(max(STEPS, WARMUP))]
    for a in actions[:WARMUP]:
        env.step(a)
    rates = []
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a in actions[:STEPS]:
            env.step(a)
        torch.cuda.synchronize()
        rates.append(N * STEPS / (time.perf_counter() - t0))
    out[mode] = dict(env_steps_per_s=rates, slowest=min(rates))
    if mode != "state":
        for uid, cam in env._sensors.items():
            def launch_ms(launch):
                ms = []
                for _ in range(RUNS):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    for _ in range(STEPS):
                        launch()
                    b.record()
                    torch.cuda.synchronize()
                    ms.append(a.elapsed_time(b) / STEPS)
                return ms

            ms = launch_ms(cam.capture)
            out[mode][uid] = dict(raycast_launch_ms=ms, slowest=max(ms), rays_per_launch=N * cam.width * cam.height)
            if args.shade:
                cam.capture_picture()  # (the colour tables are built and uploaded at the first picture)
                ms = launch_ms(cam.capture_picture)
                out[mode][uid].update(shade_launch_ms=ms, shade_mean=sum(ms) / len(ms), raycast_mean=sum(out[mode][uid]["raycast_launch_ms"]) / RUNS)
        out[mode]["shapes"] = int(env.scene.model.scalars["n_shape"])
    env.close()
    print(mode, json.dumps(out[mode]), flush=True)
print("RESULT " + json.dumps(out))
