"""VsBotVecEnv: a batch of single-agent games against a built-in opponent at device speed.

The agent's policy plays one side of every game, a table bot (stratego_env_amd.playout_policies: the policy of the weighted playouts) the
other.  One agent decision costs one logic launch -- the agent's move and the bot's reply together (sgx_step_vs) -- and ONE observation,
not the two full steps of a self-play loop.  Replaces the vs_bot branch of StrategoMultiAgentEnv (maenv:573-619), whose opponent is an
external bot behind a socket."""
import torch

from .playout_policies import capture_biased
from .procedural_env import StepVsResult, playout_weights
from .vec_env import VecStrategoEnv


class VsBotVecEnv:
    """num_envs games of `version`, the agent against `opponent`.

    opponent: a [4, 13, 14] weight table (playout_policies; default capture_biased of the variant).  agent: the agent's side, +1 / -1 for
    every game, an int8 tensor [N], or 'random' (drawn per game from a host generator seeded with `seed`, redrawn for every game that
    restarts).  see_all=True lets the bot look at the agent's true piece types; by default it sees what its partial observation shows.
    auto_reset: a finished game is reported by the step that finishes it and restarted by the same step.  seed and every other keyword
    go to the wrapped VecStrategoEnv (`env`), whose set_curriculum / set_start_states work unchanged: restarts draw from the start pool.

    reset() -> (obs, mask); step(actions) -> (obs, mask, reward, done, info).  After either, EVERY game that is not over has the agent to
    move: obs / mask are the agent's view, actions are flat (R,C,K) indices in the agent's perspective as VecStrategoEnv.step takes them.
    reward float32 [N] is the agent's (0 while the game runs); done uint8 [N]; info holds invalid_action (1 = the action was refused:
    position unchanged, the bot stayed still, play another), reply_action (the bot's move in the bot's perspective, -1 = none) and
    ending_invalid (the max-turn tie).  The result tensors are the wrapper's own and are overwritten by the next step.
    A game that the bot's OPENING move already ends (it is the bot's turn in a fresh game and its one move finishes it) is reported --
    done, reward -- by the NEXT step(), which ignores the action given for it and then restarts it.
    step() never synchronises with the host: the restart of finished games and the bot's opening call are always issued.  The bot's draws
    are keyed by (seed, env id, a call counter, turn): a run is a function of its seed."""

    def __init__(self, version='barrage', num_envs=1, opponent=None, agent=1, see_all=False, auto_reset=True, seed=0, **env_kwargs):
        env_kwargs.pop('auto_reset', None)            # (the wrapped env never steps on its own: restarts are this class's)
        self.env = VecStrategoEnv(version, num_envs, seed=seed, auto_reset=False, **env_kwargs)
        env = self.env
        self.num_envs, self.device = env.num_envs, env.device
        self.weights = playout_weights(capture_biased() if opponent is None else opponent)
        self.see_all, self.auto_reset = bool(see_all), bool(auto_reset)
        self._random_sides = isinstance(agent, str)
        self._gen = torch.Generator().manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
        if self._random_sides:
            if agent != 'random':
                raise ValueError("agent must be +1, -1, an int8 tensor [N] or 'random'")
            self.agent = self._draw_sides()
        elif isinstance(agent, int):
            if agent not in (1, -1):
                raise ValueError("agent must be +1, -1, an int8 tensor [N] or 'random'")
            self.agent = torch.full((self.num_envs,), agent, dtype=torch.int8, device=self.device)
        else:
            a = torch.as_tensor(agent).to(device=self.device, dtype=torch.int8).reshape(-1)
            if a.numel() != self.num_envs:
                raise ValueError("agent must be +1, -1, an int8 tensor [N] or 'random'")
            self.agent = torch.where(a < 0, -torch.ones_like(a), torch.ones_like(a)).contiguous()
        self._res = StepVsResult.empty(self.num_envs, self.device)
        self._open = StepVsResult.empty(self.num_envs, self.device)      # the opening calls' results: scratch
        self.reward = torch.zeros((self.num_envs,), dtype=torch.float32, device=self.device)
        self._draw = 0

    def __getattr__(self, name):                      # set_curriculum, set_start_states, obs, mask, ...: the wrapped env's
        if name == 'env':
            raise AttributeError(name)
        return getattr(self.env, name)

    def _draw_sides(self):
        s = torch.randint(0, 2, (self.num_envs,), generator=self._gen, dtype=torch.int8) * 2 - 1
        return s.to(self.device)

    def _opening(self):
        """the bot moves where a game is its to move (fresh games in which the agent is not the first mover)"""
        self.env.step_vs(None, self.agent, self.weights, see_all=self.see_all, draw=self._draw + 1, out=self._open)

    def reset(self):
        """Start every game anew, let the bot open where it moves first, and return (obs, mask) of the agent."""
        self.env.reset(observe=False)
        if self._random_sides:
            self.agent = self._draw_sides()
        self._opening()
        self._draw += 2
        obs, mask, _ = self.env.observe()
        return obs, mask

    def step(self, actions):
        """The agent's actions (int32 [N]) and the bot's replies in one launch, restarts, one observation.
        -> (obs, mask, reward float32 [N] of the agent, done uint8 [N], info)."""
        env, res = self.env, self._res
        env.step_vs(actions, self.agent, self.weights, see_all=self.see_all, draw=self._draw, out=res)
        torch.where(self.agent > 0, res.reward[:, 0], res.reward[:, 1], out=self.reward)
        if self.auto_reset:
            env.reset(env_select=res.done, observe=False)
            if self._random_sides:
                self.agent = torch.where(res.done != 0, self._draw_sides(), self.agent)
            self._opening()
        self._draw += 2
        obs, mask, _ = env.observe()
        return obs, mask, self.reward, res.done, {'invalid_action': res.invalid_action, 'reply_action': res.reply_action,
                                                  'ending_invalid': res.ending_invalid}

    def close(self):
        self.env.close()
