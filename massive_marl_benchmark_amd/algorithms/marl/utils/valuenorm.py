"""The value normaliser of the MARL trainers: the running mean, mean of squares and debiasing term of the reference's PopArt
(agents/algorithms/marl/utils/popart.py) and ValueNorm (utils/valuenorm.py).  The two reference classes keep the same state and the
same arithmetic and differ only in API, so this one class offers both: `update` / `normalize` / `denormalize` / `running_mean_var`
(ValueNorm), and calling it is PopArt's forward -- update (when train=True), then normalise.  All state stays on the device as fp32
tensors; nothing here synchronises with the host."""
import numpy as np
import torch


class ValueNorm(torch.nn.Module):
    def __init__(self, input_shape, norm_axes=1, beta=0.99999, per_element_update=False, epsilon=1e-5, device=torch.device("cpu")):
        super().__init__()
        self.input_shape = input_shape
        self.norm_axes = norm_axes
        self.epsilon = epsilon
        self.beta = beta
        self.per_element_update = per_element_update
        self.tpdv = dict(dtype=torch.float32, device=device)
        # plain tensors, as in the reference (its nn.Parameter(..).to(..) leaves tensors that are not registered either)
        self.running_mean = torch.zeros(input_shape, **self.tpdv)
        self.running_mean_sq = torch.zeros(input_shape, **self.tpdv)
        self.debiasing_term = torch.tensor(0.0, **self.tpdv)

    def reset_parameters(self):
        self.running_mean.zero_()
        self.running_mean_sq.zero_()
        self.debiasing_term.zero_()

    def _cast(self, x):
        if type(x) == np.ndarray:
            x = torch.from_numpy(x)
        return x.to(**self.tpdv)

    def running_mean_var(self):
        debiased_mean = self.running_mean / self.debiasing_term.clamp(min=self.epsilon)
        debiased_mean_sq = self.running_mean_sq / self.debiasing_term.clamp(min=self.epsilon)
        debiased_var = (debiased_mean_sq - debiased_mean ** 2).clamp(min=1e-2)
        return debiased_mean, debiased_var

    @torch.no_grad()
    def update(self, input_vector):
        x = self._cast(input_vector).detach()
        axes = tuple(range(self.norm_axes))
        batch_mean = x.mean(dim=axes)
        batch_sq_mean = (x ** 2).mean(dim=axes)
        weight = self.beta ** int(np.prod(x.size()[:self.norm_axes])) if self.per_element_update else self.beta
        self.running_mean.mul_(weight).add_(batch_mean * (1.0 - weight))
        self.running_mean_sq.mul_(weight).add_(batch_sq_mean * (1.0 - weight))
        self.debiasing_term.mul_(weight).add_(1.0 * (1.0 - weight))

    def normalize(self, input_vector):
        x = self._cast(input_vector)
        mean, var = self.running_mean_var()
        return (x - mean[(None,) * self.norm_axes]) / torch.sqrt(var)[(None,) * self.norm_axes]

    def denormalize(self, input_vector):
        """Normalised data back in the original distribution."""
        x = self._cast(input_vector)
        mean, var = self.running_mean_var()
        return (x * torch.sqrt(var)[(None,) * self.norm_axes] + mean[(None,) * self.norm_axes]).detach()

    def forward(self, input_vector, train=True):
        """PopArt.forward: the statistics take the batch in (train=True), then the batch is normalised by them."""
        if train:
            self.update(input_vector)
        return self.normalize(input_vector)


PopArt = ValueNorm
