"""The statements of the reference's Mahalanobis method (tasks/gqa_maha.py:129-183 and :223-270), kept once for the GPU test, the fixture generator
(tools/gen_g13_maha.py) and the timing tool (tools/maha_bench.py).  Only the hard-coded .cuda() calls are gone (tensors stay on the device their
caller put them on) and every intermediate is returned.  Not a test module."""
import numpy as np
import torch
from torch.autograd import Variable


def class_loop(outputs, sample_mean, precision, num_classes):
    """:228-236 / :260-268"""
    gaussian_score = 0
    for i in range(num_classes):
        batch_sample_mean = sample_mean[i]
        zero_f = outputs.data - batch_sample_mean
        term_gau = -0.5 * torch.mm(torch.mm(zero_f, precision), zero_f.t()).diag()
        if i == 0:
            gaussian_score = term_gau.view(-1, 1)
        else:
            gaussian_score = torch.cat((gaussian_score, term_gau.view(-1, 1)), 1)
    return gaussian_score


def ood_batch(model, feats, boxes, sent, sample_mean, precision, num_classes, noise):
    """:223-270 for one batch; model(feats, boxes, sent) -> (logit, pooled)"""
    feats, boxes = Variable(feats, requires_grad=True), Variable(boxes, requires_grad=True)
    _, outputs = model(feats, boxes, sent)
    gaussian_score = class_loop(outputs, sample_mean, precision, num_classes)
    # Input_processing
    sample_pred = gaussian_score.max(1)[1]
    batch_sample_mean = sample_mean.index_select(0, sample_pred)
    zero_f = outputs - Variable(batch_sample_mean)
    pure_gau = -0.5 * torch.mm(torch.mm(zero_f, Variable(precision)), zero_f.t()).diag()
    loss = torch.mean(-pure_gau)
    loss.backward()
    gradient = torch.ge(feats.grad.data, 0)
    gradient = (gradient.float() - 0.5) * 2
    featsPt = torch.add(feats.data, gradient, alpha=-noise)
    gradient = torch.ge(boxes.grad.data, 0)
    gradient = (gradient.float() - 0.5) * 2
    boxesPt = torch.add(boxes.data, gradient, alpha=-noise)
    with torch.no_grad():
        _, noised_outputs = model(Variable(featsPt), Variable(boxesPt), sent)
        noised_gaussian_score = class_loop(noised_outputs, sample_mean, precision, num_classes)
        score, label = torch.max(noised_gaussian_score, dim=1)
    return dict(pooled=outputs.detach(), gaussian_score=gaussian_score, sample_pred=sample_pred, loss=loss.detach(), dfeats=feats.grad, dboxes=boxes.grad,
                pooled2=noised_outputs, noised_gaussian_score=noised_gaussian_score, score2=score, label2=label)


def sample_estimator(model, loader, num_classes):
    """:129-183; loader yields (feats, boxes, sent, target) with the UQ column already dropped (:141).  Needs sklearn.
    Returns (sample_class_mean, precision, num_sample_per_class, the pooled rows, the fitted covariance)."""
    import sklearn.covariance
    group_lasso = sklearn.covariance.EmpiricalCovariance(assume_centered=False)
    num_sample_per_class = np.zeros((num_classes))
    list_features = [0 for i in range(num_classes)]
    model.eval()
    rows = []
    with torch.no_grad():
        for feats, boxes, sent, target in loader:
            _, outputs = model(feats, boxes, sent)
            outputs = outputs.cpu()
            rows.append(outputs.numpy().copy())
            for i in range(target.size(0)):
                for j in range(num_classes):
                    if target[i][j] == 0:
                        continue
                    label = j
                    if num_sample_per_class[label] == 0:
                        list_features[label] = outputs[i].view(1, -1)
                    else:
                        list_features[label] = torch.cat([list_features[label], outputs[i].view(1, -1)], 0)
                    num_sample_per_class[label] += 1
        sample_class_mean = torch.zeros((num_classes, outputs.size(1)))
        for j in range(num_classes):
            if isinstance(list_features[j], torch.Tensor):
                sample_class_mean[j] = torch.mean(list_features[j], 0)
        X = []
        for i in range(num_classes):
            if isinstance(list_features[i], torch.Tensor):
                X.append(list_features[i] - sample_class_mean[i])
        X = torch.cat(X, 0)
        # find inverse
        group_lasso.fit(X.numpy())
        precision = group_lasso.precision_
    return sample_class_mean, precision, num_sample_per_class, np.concatenate(rows, 0), group_lasso.covariance_
