"""MAPPO_Policy, HAPPO_Policy, HATRPO_Policy: one agent's Actor and Critic (actor_critic.py) with their Adam optimizers, under the
reference's constructor `(config, obs_space, cent_obs_space, act_space, device)`, attributes (`actor`, `critic`, `actor_optimizer`,
`critic_optimizer`, `lr`, `critic_lr`, `opti_eps`, `weight_decay`, `obs_space`, `share_obs_space`, `act_space`) and methods
(agents/algorithms/marl/mappo_policy.py, happo_policy.py, hatrpo_policy.py) -- what trainer.MAPPO / HAPPO, hatrpo.HATRPO,
GroupedPolicyInference.from_trainers and runner.Runner take as `policy`.

The three differ in one place: HATRPO's evaluate_actions passes on the five values its Actor returns (log-probabilities, entropy, the
distribution's mean and std, and None for a Discrete space's logits) behind the values; the other two return
(values, action_log_probs, dist_entropy).  The Actor looks at config["algorithm_name"] for that, as the reference's does."""
import torch

from .actor_critic import Actor, Critic


def update_linear_schedule(optimizer, epoch, total_num_epochs, initial_lr):
    """The learning rate falls linearly from initial_lr at epoch 0 to 0 at total_num_epochs"""
    lr = initial_lr - initial_lr * (epoch / float(total_num_epochs))
    for group in optimizer.param_groups:
        group["lr"] = lr


class _Policy:
    def __init__(self, config, obs_space, cent_obs_space, act_space, device=torch.device("cpu")):
        self.config = self.args = config
        self.device = device
        self.lr = config["lr"]
        self.critic_lr = config["critic_lr"]
        self.opti_eps = config["opti_eps"]
        self.weight_decay = config["weight_decay"]
        self.obs_space = obs_space
        self.share_obs_space = cent_obs_space
        self.act_space = act_space
        self.actor = Actor(config, self.obs_space, self.act_space, self.device)
        self.critic = Critic(config, self.share_obs_space, self.device)
        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr=self.lr, eps=self.opti_eps, weight_decay=self.weight_decay)
        self.critic_optimizer = torch.optim.Adam(self.critic.parameters(), lr=self.critic_lr, eps=self.opti_eps, weight_decay=self.weight_decay)

    def lr_decay(self, episode, episodes):
        update_linear_schedule(self.actor_optimizer, episode, episodes, self.lr)
        update_linear_schedule(self.critic_optimizer, episode, episodes, self.critic_lr)

    def get_actions(self, cent_obs, obs, rnn_states_actor, rnn_states_critic, masks, available_actions=None, deterministic=False):
        """(values, actions, action_log_probs, rnn_states_actor, rnn_states_critic)"""
        actions, action_log_probs, rnn_states_actor = self.actor(obs, rnn_states_actor, masks, available_actions, deterministic)
        values, rnn_states_critic = self.critic(cent_obs, rnn_states_critic, masks)
        return values, actions, action_log_probs, rnn_states_actor, rnn_states_critic

    def get_values(self, cent_obs, rnn_states_critic, masks):
        return self.critic(cent_obs, rnn_states_critic, masks)[0]

    def evaluate_actions(self, cent_obs, obs, rnn_states_actor, rnn_states_critic, action, masks, available_actions=None, active_masks=None):
        """(values, *what the Actor's evaluate_actions returns): three values, six for HATRPO"""
        evaluated = self.actor.evaluate_actions(obs, rnn_states_actor, action, masks, available_actions, active_masks)
        values, _ = self.critic(cent_obs, rnn_states_critic, masks)
        return (values,) + tuple(evaluated)

    def act(self, obs, rnn_states_actor, masks, available_actions=None, deterministic=False):
        actions, _, rnn_states_actor = self.actor(obs, rnn_states_actor, masks, available_actions, deterministic)
        return actions, rnn_states_actor


class MAPPO_Policy(_Policy):
    pass


class HAPPO_Policy(_Policy):
    pass


class HATRPO_Policy(_Policy):
    def __init__(self, config, obs_space, cent_obs_space, act_space, device=torch.device("cpu")):
        if config["algorithm_name"] != "hatrpo":
            raise ValueError("HATRPO_Policy: config['algorithm_name'] must be 'hatrpo' (the Actor returns the distribution's mean and std for it)")
        super().__init__(config, obs_space, cent_obs_space, act_space, device)
