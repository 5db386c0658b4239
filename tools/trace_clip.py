"""fb_vec_step of 'double' on the dueling 512 / 2 net, 1024 envs, B = 32, with or without a gradient-norm limit and soft target updates --
target for rocprofv3 --kernel-trace; tools/trace_gaps.py on the CSV then gives the in-situ duration of every kernel of a step and the idle
gap in front of it.  FB_TRACE_CLIP=G (0 = off), FB_TRACE_POLYAK=rho (0 = off), FB_TRACE_SPLIT=0 keeps the unclipped step on one stream
(what a clipped step is compared with launch by launch), FB_TRACE_ALGO=doubleper takes a prioritized memory."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dqnflappybird_amd import _lib as L
from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep
n, B = int(os.environ.get("FB_TRACE_ENVS", "1024")), 32
algo = os.environ.get("FB_TRACE_ALGO", "double")
G, rho = float(os.environ.get("FB_TRACE_CLIP", "0")), float(os.environ.get("FB_TRACE_POLYAK", "0"))
per = algo == "doubleper"
env, replay, net = VecGameState(n, seed=0), VecReplay(1_000_000, n, prioritized=per), QNet(2, 512, "dueling", max_batch=n)
replay.seed(0, "numpy" if per else "cpython")
net.init_params(0, which=0); net.init_params(1, which=1)
net.set_max_grad_norm(G)
L.check(L.lib().fb_vec_step_set_schedule(int(os.environ.get("FB_TRACE_SPLIT", "1"))), "fb_vec_step_set_schedule")
env.track_state(); env.observe(); replay.reset(env.frame_bits)
one = VecStep(env, replay, net, B, algo)
for step in range(int(os.environ.get("FB_TRACE_STEPS", "400"))):
    one(0.03, seed=0, step=step, train=True)
    if rho:
        net.soft_sync_target(rho)
torch.cuda.synchronize()
print("split schedule:", net.split_stats(), " last clip:", net.grad_norm())
