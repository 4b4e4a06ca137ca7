from .stepper import ReduceToBason
