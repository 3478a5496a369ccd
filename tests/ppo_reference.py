"""A numpy restatement, written fresh, of the reference's rollout buffer: `Experience.store`, `sort_training_data` and
`flatten_batch` (gpudrive/integrations/puffer/ppo.py:530-666) with the Python `sorted` on (env_id, step) tuples kept as it is,
and the serial GAE loop in np.float32 scalars (the rule DESIGN.md states; pufferlib's c_gae source is not available).  The
yardstick of tests/test_rollout.py and tests/test_gpu_rollout.py."""
import numpy as np


class Experience:
    def __init__(self, batch_size, minibatch_size=None, bptt_horizon=1, *, obs_width, action_shape=()):
        if minibatch_size is None:
            minibatch_size = batch_size
        num_minibatches = batch_size / minibatch_size
        self.num_minibatches = int(num_minibatches)
        if self.num_minibatches != num_minibatches:
            raise ValueError("batch_size must be divisible by minibatch_size")
        minibatch_rows = minibatch_size / bptt_horizon
        self.minibatch_rows = int(minibatch_rows)
        if self.minibatch_rows != minibatch_rows:
            raise ValueError("minibatch_size must be divisible by bptt_horizon")
        self.batch_size, self.bptt_horizon, self.minibatch_size = batch_size, bptt_horizon, minibatch_size
        self.obs = np.zeros((batch_size, obs_width), np.float32)
        self.actions = np.zeros((batch_size,) + tuple(action_shape), np.int64)
        self.logprobs = np.zeros(batch_size, np.float32)
        self.rewards = np.zeros(batch_size, np.float32)
        self.dones = np.zeros(batch_size, np.float32)
        self.values = np.zeros(batch_size, np.float32)
        self.sort_keys = []
        self.ptr = 0
        self.step = 0
        self.dropped = 0  # (not the reference's: live rows its slice cut off)

    @property
    def full(self):
        return self.ptr >= self.batch_size

    def store(self, obs, value, action, logprob, reward, done, env_id, mask):
        ptr = self.ptr
        live = np.where(mask)[0]
        indices = live[: self.batch_size - ptr]
        end = ptr + len(indices)
        self.obs[ptr:end] = obs[indices]
        self.values[ptr:end] = np.asarray(value).reshape(-1)[indices]
        self.actions[ptr:end] = action[indices]
        self.logprobs[ptr:end] = logprob[indices]
        self.rewards[ptr:end] = reward[indices]
        self.dones[ptr:end] = done[indices]
        self.sort_keys.extend([(env_id[i], self.step) for i in indices])
        self.dropped += len(live) - len(indices)
        self.ptr = end
        self.step += 1

    def sort_training_data(self):
        idxs = np.asarray(sorted(range(len(self.sort_keys)), key=self.sort_keys.__getitem__))
        self.b_idxs = idxs.reshape(self.minibatch_rows, self.num_minibatches, self.bptt_horizon).transpose(1, 0, 2)
        self.b_idxs_flat = self.b_idxs.reshape(self.num_minibatches, self.minibatch_size)
        self.sort_keys = []
        self.ptr = 0
        self.step = 0
        return idxs

    def flatten_batch(self, advantages):
        b_idxs, b_flat = self.b_idxs, self.b_idxs_flat
        self.b_advantages = (advantages.reshape(self.minibatch_rows, self.num_minibatches, self.bptt_horizon)
                             .transpose(1, 0, 2).reshape(self.num_minibatches, self.minibatch_size))
        self.b_obs = self.obs[b_idxs]
        self.b_actions = self.actions[b_idxs]
        self.b_logprobs = self.logprobs[b_idxs]
        self.b_dones = self.dones[b_idxs]
        self.b_values = self.values[b_flat]
        self.b_returns = self.b_advantages + self.b_values  # float32 + float32: one fp32 add
        return (self.b_obs, self.b_actions, self.b_logprobs, self.b_dones, self.b_values, self.b_advantages, self.b_returns)


def compute_gae(dones, values, rewards, gamma, gae_lambda):
    """The serial loop over the sorted batch, every operation a rounded np.float32 one, in the stated order."""
    f = np.float32
    d, v, r = (np.asarray(x, f) for x in (dones, values, rewards))
    n = len(d)
    gamma, gae_lambda = f(gamma), f(gae_lambda)
    adv = np.zeros(n, f)
    last = f(0)
    one = f(1)
    with np.errstate(all="ignore"):
        for t in range(n - 2, -1, -1):
            nnt = one - d[t + 1]
            delta = (r[t + 1] + ((gamma * v[t + 1]) * nnt)) - v[t]
            last = delta + (((gamma * gae_lambda) * nnt) * last)
            adv[t] = last
    return adv


def offset_ord_permutation(rows, num_rows):
    """The device's way to the sorted order: entry p of row rows[p] is the ord[p]-th of its row, its sorted place is
    offset[row] + ord with offset the exclusive prefix sum of the per-row counts."""
    rows = np.asarray(rows, np.int64)
    count = np.zeros(num_rows, np.int64)
    ord_ = np.zeros(len(rows), np.int64)
    for p, r in enumerate(rows):
        ord_[p] = count[r]
        count[r] += 1
    offset = np.cumsum(count) - count
    idxs = np.full(len(rows), -1, np.int64)
    idxs[offset[rows] + ord_] = np.arange(len(rows))
    return idxs
