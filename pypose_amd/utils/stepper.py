"""Loop steppers (reference pypose/utils/stepper.py): the stopping rules of iterative modules such as ``pp.module.ICP``."""
import torch


class ReduceToBason:
    """Stops a loop when the loss has stopped falling: ``while stepper.continual(): ...; stepper.step(loss)``.

    A step counts towards ``patience`` when the relative decrease ``(last - loss) / loss`` is below ``decreasing``; any step
    that decreases more resets the count.  The loop ends when the count reaches ``patience``, when ``steps`` steps were taken,
    or when the loss is below ``tol``.  A batched loss has to satisfy a rule in every element.  Call ``reset()`` before a
    stepper is used again.  ``verbose`` prints the loss of every step and the rule that ended the loop, in the reference's
    words."""

    def __init__(self, steps, patience=5, decreasing=1e-3, tol=1e-5, verbose=False):
        self.max_steps, self.patience, self.decreasing, self.tol, self.verbose = steps, patience, decreasing, tol, verbose
        self.reset()

    def reset(self):
        self.last = torch.tensor(float('inf'))
        self.steps, self.patience_count, self._continual = 0, 0, True

    def continual(self):
        return self._continual

    def _quit(self, why):
        self._continual = False
        if self.verbose:
            print(f"ReduceToBason: {why}, Quiting..")

    def step(self, loss):
        if self.verbose:
            print('ReduceToBason step', self.steps, 'loss', loss)
        loss = loss if torch.is_tensor(loss) else torch.tensor(loss)
        self.steps += 1
        if torch.all(loss < self.tol):
            self._quit("Loss tol reached")
        if self.steps >= self.max_steps:
            self._quit("Maximum steps reached")
        stalled = torch.all((self.last.to(loss.device) - loss) / loss < self.decreasing)
        self.patience_count = self.patience_count + 1 if stalled else 0
        self.last = loss
        if self.patience_count >= self.patience:
            self._quit("Maximum patience steps reached")
