"""Bernoulli Thompson sampling over the d x d x d grid of Euler-angle intervals — mirror of the reference's
``attack/ISO/thompson_sample.py`` (same names and signatures). The posterior and its draws are numpy on the host and use
the GLOBAL numpy generator in the reference's call order; the device is taken from the tensors, not from a module global.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import isometry_init


def logits_info(obj, label, model):
    """(victim output, correct 0/1, probabilities sorted descending, their classes) of ONE cloud obj [1,3,N]. The softmax
    is taken on whatever the victim returns (log-probabilities for these victims), as the reference does (:9-19)."""
    with torch.no_grad():
        logits = model(obj)[0]
        rates, indices = F.softmax(logits, dim=1).sort(1, descending=True)
    rates, indices = rates.squeeze(0), indices.squeeze(0)
    return logits, int((indices[0] == label.reshape(-1)[0]).item()), rates, indices


class environment():
    """The arms: interval (i, j, k) of the cube [a0, b0]^3 cut d times per axis (:22-53). `thetas` is drawn at
    construction as in the reference (d^3 uniforms from the global numpy generator) although nothing reads it."""

    def __init__(self, d=8, a0=0, b0=2 * np.pi, train=False):
        self.d, self.a0, self.b0 = d, a0, b0
        self.generate_thetas()
        self.timestep = 0
        self.rewards = np.zeros((d, d, d))
        self.train = train

    def generate_thetas(self):
        self.thetas = np.random.uniform(0, 1, pow(self.d, 3)).reshape(self.d, self.d, self.d)

    def arm_to_interval(self, arm):
        a, b = np.zeros(3), np.zeros(3)
        for i in range(3):
            a[i] = self.a0 + (self.b0 - self.a0) * arm[i] / self.d
            b[i] = self.a0 + (self.b0 - self.a0) * (arm[i] + 1) / self.d
        return a, b

    def reward_of(self, correct):
        """Attacking, a wrong prediction pays; with train=True a right one does (:49-52)."""
        return correct if self.train else 1 - correct

    def get_reward_matrix(self, arm, obj, label, model):
        a, b = self.arm_to_interval(arm)
        matrix = isometry_init.rotation_xyz(a, b)
        model.iso.weight.data = torch.as_tensor(matrix, dtype=torch.float32).to(obj.device)
        return self.reward_of(logits_info(obj, label, model)[1]), matrix


class BetaAlgo():
    """Beta(1, 1) priors per arm and the conjugate update (:56-71)."""

    def __init__(self, environment):
        self.environment = environment
        self.d = environment.d
        self.alpha = np.ones((self.d, self.d, self.d))
        self.beta = np.ones((self.d, self.d, self.d))

    def get_reward_matrix(self, arm, obj, label, model):
        reward, matrix = self.environment.get_reward_matrix(arm, obj, label, model)
        self._update_params(arm, reward)
        return reward, matrix

    def _update_params(self, arm, reward):
        self.alpha[arm] += reward
        self.beta[arm] += 1 - reward


class BernThompson(BetaAlgo):
    def __init__(self, environment):
        super().__init__(environment)

    def get_action(self):
        """One Beta draw per arm over the whole table, then the arg-max arm (:78-81)."""
        theta = np.random.beta(self.alpha, self.beta)
        return np.unravel_index(np.argmax(theta, axis=None), theta.shape)
