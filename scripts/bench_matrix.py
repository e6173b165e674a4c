"""env-steps/s of the BASELINE.json single-GPU configurations under the reference harness's protocol: 1000 steps without a
reset (gpu_sim.py:96-106) and 1000 steps with a reset every 200 (gpu_sim.py:166-178), warm-up reset / step / reset
(gpu_sim.py:91-93); one JSON line per configuration. The 200-step figure is the first fifth of the same unreset run."""
import sys, os, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import maniskill_amd.envs  # noqa
import gymnasium as gym

def action_source(base, N, adim, control_mode):
    """random actions in [-1, 1]; `pd_ee_pose` (absolute, raw columns) gets ONE fixed reachable pose instead: the TCP's
    start pose in the root frame, 5 cm higher, as position + XYZ Euler angles, and a random gripper column"""
    if control_mode != "pd_ee_pose":
        return lambda: 2 * torch.rand(N, adim, device="cuda") - 1
    P = base.agent.controller.controllers["arm"].ee_pose_at_base.raw_pose
    w, x, y, z = P[:, 3], P[:, 4], P[:, 5], P[:, 6]
    euler = torch.stack([torch.atan2(-2 * (y * z - w * x), 1 - 2 * (x * x + y * y)), torch.asin((2 * (x * z + w * y)).clamp(-1, 1)),
                         torch.atan2(-2 * (x * y - w * z), 1 - 2 * (y * y + z * z))], 1)
    pose = torch.cat([P[:, :3] + torch.tensor([0.0, 0.0, 0.05], device=P.device), euler], 1)
    return lambda: torch.cat([pose, 2 * torch.rand(N, adim - 6, device="cuda") - 1], 1)

def run(env_id, N, steps=1000, control_mode="pd_joint_delta_pos", **kw):
    torch.manual_seed(2022)
    env = gym.make(env_id, num_envs=N, obs_mode="state", control_mode=control_mode, **kw)
    base = env.unwrapped
    adim = base.single_action_space.shape[0]
    env.reset(seed=2022)
    act = action_source(base, N, adim, control_mode)
    env.step(act())
    env.reset(seed=2022)
    torch.cuda.synchronize(); t = time.perf_counter()
    dt_200 = None
    for i in range(steps):
        env.step(act())
        if i == 199:
            torch.cuda.synchronize(); dt_200 = time.perf_counter() - t
    torch.cuda.synchronize(); dt_step = time.perf_counter() - t
    overflow = base.scene.px.overflow_count()
    env.reset(seed=2022)
    torch.cuda.synchronize(); t = time.perf_counter()
    for i in range(steps):
        env.step(act())
        if (i + 1) % 200 == 0:
            env.reset()
    torch.cuda.synchronize(); dt_reset = time.perf_counter() - t
    out = dict(env_id=env_id + (":fetch" if kw.get("robot_uids") == "fetch" or env_id.startswith("SceneManipulation") else ""), num_envs=N, control_mode=control_mode, substeps=base._sim_steps_per_control, steps=steps, step_only=round(N * steps / dt_step),
               step_only_first_200=round(N * 200 / dt_200) if dt_200 else None, step_reset_every_200=round(N * steps / dt_reset),
               ms_per_step=round(dt_step / steps * 1e3, 3), fused=base._use_fused_callers, overflow_envs=overflow + base.scene.px.overflow_count())
    print(json.dumps(out), flush=True)
    env.close()

only = sys.argv[1:]
for args, kw in ((("PickCube-v1", 4096), {}), (("PushCube-v1", 4096), {}), (("PegInsertionSide-v1", 2048), {}),
                 (("PickCube-v1", 4096), dict(control_mode="pd_ee_delta_pos")), (("PickCube-v1", 4096), dict(control_mode="pd_ee_delta_pose")),
                 # the modes that track a target pose: the iterative-IK block of the action map (MS_FUSED=0: the torch solver)
                 (("PickCube-v1", 4096), dict(control_mode="pd_ee_target_delta_pos")), (("PickCube-v1", 4096), dict(control_mode="pd_ee_target_delta_pose")),
                 (("PickCube-v1", 4096), dict(control_mode="pd_ee_pose")),
                 (("PickCube-v1", 16384), {}),
                 (("StackCube-v1", 4096), {}),  # two cubes: the two-row control-step kernel (MS_FUSED=0: the torch epilogue)
                 (("PushT-v1", 4096), {}),  # panda_stick + T block: k_solve16<7, 5> with the pseudo-render at its tail (MS_FUSED=0: torch)
                 # the plain one-row control step + the epilogue as a launch of its own (MS_FUSED=0: the torch epilogue)
                 (("RollBall-v1", 4096), {}), (("PullCube-v1", 4096), {}),
                 # the same on the two-row control step (peg + cube: 21 velocity components) and on one row, both with grasp detection
                 (("PokeCube-v1", 4096), {}), (("LiftPegUpright-v1", 4096), {}),
                 # place-and-release against a five-box kinematic bin (one row), and panda_wristcam + cube + two-box tool (two rows)
                 (("PlaceSphere-v1", 4096), {}), (("PullCubeTool-v1", 4096), {}),
                 # millimetre geometry: 1.5 mm pegs and a five-box receptacle (one row; the epilogue reads the env's stored goal).
                 # `plug` selects this row alone and runs it twice in one process: native, then MS_FUSED=0 (the torch epilogue)
                 (("PlugCharger-v1", 4096), {}),
                 # panda_stick on a canvas: the plain one-row step <7, 0> (4 position sweeps, no velocity sweep) + the dot layer /
                 # evaluate epilogue. `draw` selects this row alone and runs it twice as `plug` does. The unreset 1000 steps run
                 # past the 300-dot table: from step 300 on the epilogue appends nothing
                 (("DrawTriangle-v1", 4096), {}),
                 (("PickCube-v1", 4096), dict(sim_config=dict(control_freq=25))),  # 4 substeps (SURVEY 8d reports 5 and 4)
                 # BASELINE config 5's robot and env count: the Fetch on an empty ground, and in synthetic triangle-mesh rooms
                 (("Empty-v1", 1024), dict(robot_uids="fetch")), (("SceneManipulation-v1", 1024), dict(build_config_idxs=[i % 5 for i in range(1024)])),
                 # the Fetch's end-effector modes: base and torso are on the gripper's path and held by the two blocks
                 # (`fetch_ee` selects these four rows alone; MS_FUSED=0: the torch solver)
                 *((("Empty-v1", 1024), dict(robot_uids="fetch", control_mode=m))
                   for m in ("pd_ee_delta_pos", "pd_ee_delta_pose", "pd_ee_target_delta_pos", "pd_ee_target_delta_pose")),
                 # table-top tasks with the Fetch: the two-row 15-dof plain control step + the epilogue under the Fetch's robot
                 # profile as a launch of its own (`fetch_tabletop` selects these two rows alone; MS_FUSED=0: the torch epilogue)
                 (("PickCube-v1", 4096), dict(robot_uids="fetch")), (("PullCubeTool-v1", 4096), dict(robot_uids="fetch"))):
    fetch_ee = kw.get("robot_uids") == "fetch" and "control_mode" in kw
    fetch_tabletop = kw.get("robot_uids") == "fetch" and args[0] != "Empty-v1"
    if ("fetch_ee" in only and not fetch_ee) or (fetch_tabletop and only and "fetch_tabletop" not in only):
        continue
    if fetch_tabletop and "fetch_tabletop" in only:
        run(*args, **kw)
        continue
    if ("plug" in only and args[0] == "PlugCharger-v1") or ("draw" in only and args[0] == "DrawTriangle-v1"):
        before = os.environ.get("MS_FUSED")
        for fused in ("1", "0"):  # (read when the env is made; each line's `fused` says which path ran)
            os.environ["MS_FUSED"] = fused
            run(*args, **kw)
        os.environ.pop("MS_FUSED") if before is None else os.environ.__setitem__("MS_FUSED", before)
        continue
    if not only or args[0] in only or kw.get("control_mode") in only or ("substeps4" in only and "sim_config" in kw) or ("fetch_ee" in only and fetch_ee):
        run(*args, **kw)
