"""Invertible image transforms for test-time augmentation (reference ever/interface/transform_base.py): a `Transform` maps a
[batch, channel, height, width] tensor to its augmented view and a model output on that view back; a `MultiTransform`
applies a list of them."""
import numpy as np
import torch


class Transform(object):
    def __init__(self):
        pass

    def transform(self, inputs):
        """inputs: 4-D tensor [batch, channel, height, width] -> transformed_inputs"""
        raise NotImplementedError

    def inv_transform(self, transformed_inputs):
        """the inverse: transformed_inputs -> inputs"""
        raise NotImplementedError

    @staticmethod
    def unit_test(transform):
        inputs = torch.ones(2, 32, 128, 128)
        back = transform.inv_transform(transform.transform(inputs))
        np.testing.assert_almost_equal(back.numpy(), inputs.numpy())


class MultiTransform(list):
    def __init__(self, *transforms):
        super(MultiTransform, self).__init__()
        assert all([isinstance(t, Transform) for t in transforms])
        self._trans_list = transforms

    def transform(self, inputs):
        """one transformed copy of `inputs` per transform"""
        return [t.transform(inputs) for t in self._trans_list]

    def inv_transform(self, transformed_inputs):
        """every element taken back by its own transform"""
        return [t.inv_transform(ti) for ti, t in zip(transformed_inputs, self._trans_list)]
