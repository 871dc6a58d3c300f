"""The Keras callbacks RetinaNet.py's create_callbacks builds (RetinaNet.py:136-193): ModelCheckpoint, EarlyStopping,
ReduceLROnPlateau, LearningRateScheduler and CSVLogger, for Model.fit_generator (model/defineModel.py).

Keras is not a dependency of this package, so the rules of Keras 2.x (keras/callbacks.py, 2.2.x - the reference's `import keras`)
are restated here, each in its class's docstring, and pinned by tests/test_callbacks.py.  fit_generator calls, in list order,
set_model once, on_train_begin, then per epoch on_epoch_begin / on_epoch_end (with the epoch's `logs` dict, which callbacks may
add to for the ones after them), and on_train_end.  The learning rate lives in `model.optimizer.lr` (a plain float here, where Keras
holds a backend variable), which the training step reads every batch."""
import csv
import os
import warnings
from collections import OrderedDict

import numpy as np


class Callback:
    """keras.callbacks.Callback: holds `model` (set_model) and `params`, and has every hook as a no-op."""

    def __init__(self):
        self.model = None
        self.params = None

    def set_params(self, params):
        self.params = params

    def set_model(self, model):
        self.model = model

    def on_train_begin(self, logs=None):
        pass

    def on_train_end(self, logs=None):
        pass

    def on_epoch_begin(self, epoch, logs=None):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass

    def on_batch_begin(self, batch, logs=None):
        pass

    def on_batch_end(self, batch, logs=None):
        pass


def _auto_is_max(monitor, fmeasure=False):
    """Keras' `auto` mode: maximise when the monitored name contains 'acc' (ModelCheckpoint: or starts with 'fmeasure'),
    minimise anything else - 'mAP' included, so select by mAP with mode='max'."""
    return 'acc' in monitor or (fmeasure and monitor.startswith('fmeasure'))


def _mode(mode, monitor, who, fmeasure=False):
    if mode not in ('auto', 'min', 'max'):
        warnings.warn('%s mode %s is unknown, fallback to auto mode.' % (who, mode), RuntimeWarning)
        mode = 'auto'
    if mode == 'auto':
        mode = 'max' if _auto_is_max(monitor, fmeasure) else 'min'
    return mode


class ModelCheckpoint(Callback):
    """keras.callbacks.ModelCheckpoint(filepath, monitor='val_loss', verbose=0, save_best_only=False, save_weights_only=False,
    mode='auto', period=1).

    Every `period` epochs (counted since the last save attempt) the path is filepath.format(epoch=epoch + 1, **logs) - so
    '{epoch:02d}' is 1-based and any key of the logs may appear.  save_best_only: the monitored value must beat the best so far
    (np.less for min, np.greater for max; the best starts at +/- infinity; equal is no improvement); a monitored value missing
    from the logs warns (RuntimeWarning, 'Can save best model only with <monitor> available, skipping.') and saves nothing.
    save_weights_only selects model.save_weights over model.save."""

    def __init__(self, filepath, monitor='val_loss', verbose=0, save_best_only=False, save_weights_only=False, mode='auto', period=1):
        super(ModelCheckpoint, self).__init__()
        self.filepath, self.monitor, self.verbose = filepath, monitor, verbose
        self.save_best_only, self.save_weights_only, self.period = save_best_only, save_weights_only, period
        self.epochs_since_last_save = 0
        self.mode = _mode(mode, monitor, 'ModelCheckpoint', fmeasure=True)
        self.monitor_op = np.greater if self.mode == 'max' else np.less
        self.best = -np.inf if self.mode == 'max' else np.inf

    def _save(self, filepath):
        if self.save_weights_only:
            self.model.save_weights(filepath)
        else:
            self.model.save(filepath)

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        self.epochs_since_last_save += 1
        if self.epochs_since_last_save < self.period:
            return
        self.epochs_since_last_save = 0
        filepath = self.filepath.format(epoch=epoch + 1, **logs)
        if not self.save_best_only:
            if self.verbose > 0:
                print('\nEpoch %05d: saving model to %s' % (epoch + 1, filepath))
            self._save(filepath)
            return
        current = logs.get(self.monitor)
        if current is None:
            warnings.warn('Can save best model only with %s available, skipping.' % self.monitor, RuntimeWarning)
        elif self.monitor_op(current, self.best):
            if self.verbose > 0:
                print('\nEpoch %05d: %s improved from %0.5f to %0.5f, saving model to %s'
                      % (epoch + 1, self.monitor, self.best, current, filepath))
            self.best = current
            self._save(filepath)
        elif self.verbose > 0:
            print('\nEpoch %05d: %s did not improve from %0.5f' % (epoch + 1, self.monitor, self.best))


class EarlyStopping(Callback):
    """keras.callbacks.EarlyStopping(monitor='val_loss', min_delta=0, patience=0, verbose=0, mode='auto', baseline=None).

    on_train_begin resets: wait = 0, stopped_epoch = 0, best = baseline if given else +/- infinity.  An epoch improves when
    monitor_op(current - min_delta, best) with min_delta signed by the direction (|min_delta| for max, -|min_delta| for min);
    it then becomes the best and wait returns to 0.  Otherwise wait += 1 and, once wait >= patience, stopped_epoch = epoch and
    model.stop_training = True.  A missing monitored value warns and changes nothing.  (restore_best_weights is not offered.)"""

    def __init__(self, monitor='val_loss', min_delta=0, patience=0, verbose=0, mode='auto', baseline=None):
        super(EarlyStopping, self).__init__()
        self.monitor, self.patience, self.verbose, self.baseline = monitor, patience, verbose, baseline
        self.mode = _mode(mode, monitor, 'EarlyStopping')
        self.monitor_op = np.greater if self.mode == 'max' else np.less
        self.min_delta = abs(min_delta) if self.mode == 'max' else -abs(min_delta)
        self.wait = 0
        self.stopped_epoch = 0
        self.best = None

    def on_train_begin(self, logs=None):
        self.wait = 0
        self.stopped_epoch = 0
        if self.baseline is not None:
            self.best = self.baseline
        else:
            self.best = -np.inf if self.mode == 'max' else np.inf

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        current = logs.get(self.monitor)
        if current is None:
            warnings.warn('Early stopping conditioned on metric `%s` which is not available. Available metrics are: %s'
                          % (self.monitor, ','.join(list(logs.keys()))), RuntimeWarning)
            return
        if self.best is None:
            self.on_train_begin()
        if self.monitor_op(current - self.min_delta, self.best):
            self.best = current
            self.wait = 0
        else:
            self.wait += 1
            if self.wait >= self.patience:
                self.stopped_epoch = epoch
                self.model.stop_training = True

    def on_train_end(self, logs=None):
        if self.stopped_epoch > 0 and self.verbose > 0:
            print('Epoch %05d: early stopping' % (self.stopped_epoch + 1))


class ReduceLROnPlateau(Callback):
    """keras.callbacks.ReduceLROnPlateau(monitor='val_loss', factor=0.1, patience=10, verbose=0, mode='auto', min_delta=1e-4,
    cooldown=0, min_lr=0).  factor >= 1 is a ValueError.

    on_train_begin resets best (+/- infinity), wait and the cooldown counter.  on_epoch_end first writes logs['lr'] = the
    current rate, then: in cooldown, the counter goes down by one and wait = 0; an improvement (current < best - min_delta for
    min, current > best + min_delta for max) becomes the best with wait = 0; otherwise, outside cooldown, wait += 1 and once
    wait >= patience a rate above min_lr becomes max(rate * factor, min_lr), the cooldown counter is set to `cooldown` and
    wait = 0 (a rate already at min_lr stays, and wait keeps counting).  A missing monitored value warns."""

    def __init__(self, monitor='val_loss', factor=0.1, patience=10, verbose=0, mode='auto', min_delta=1e-4, cooldown=0, min_lr=0):
        super(ReduceLROnPlateau, self).__init__()
        if factor >= 1.0:
            raise ValueError('ReduceLROnPlateau does not support a factor >= 1.0.')
        self.monitor, self.factor, self.patience, self.verbose = monitor, factor, patience, verbose
        self.min_delta, self.cooldown, self.min_lr = min_delta, cooldown, min_lr
        self.mode = _mode(mode, monitor, 'Learning Rate Plateau Reducing')
        self._reset()

    def _reset(self):
        if self.mode == 'max':
            self.monitor_op = lambda a, b: np.greater(a, b + self.min_delta)
            self.best = -np.inf
        else:
            self.monitor_op = lambda a, b: np.less(a, b - self.min_delta)
            self.best = np.inf
        self.cooldown_counter = 0
        self.wait = 0

    def in_cooldown(self):
        return self.cooldown_counter > 0

    def on_train_begin(self, logs=None):
        self._reset()

    def on_epoch_end(self, epoch, logs=None):
        logs = logs if logs is not None else {}
        logs['lr'] = float(self.model.optimizer.lr)
        current = logs.get(self.monitor)
        if current is None:
            warnings.warn('Reduce LR on plateau conditioned on metric `%s` which is not available. Available metrics are: %s'
                          % (self.monitor, ','.join(list(logs.keys()))), RuntimeWarning)
            return
        if self.in_cooldown():
            self.cooldown_counter -= 1
            self.wait = 0
        if self.monitor_op(current, self.best):
            self.best = current
            self.wait = 0
        elif not self.in_cooldown():
            self.wait += 1
            if self.wait >= self.patience:
                old_lr = float(self.model.optimizer.lr)
                if old_lr > self.min_lr:
                    new_lr = max(old_lr * self.factor, self.min_lr)
                    self.model.optimizer.lr = new_lr
                    if self.verbose > 0:
                        print('\nEpoch %05d: ReduceLROnPlateau reducing learning rate to %s.' % (epoch + 1, new_lr))
                    self.cooldown_counter = self.cooldown
                    self.wait = 0


class LearningRateScheduler(Callback):
    """keras.callbacks.LearningRateScheduler(schedule, verbose=0): on_epoch_begin sets the rate to schedule(epoch, lr) - or
    schedule(epoch) for a one-argument function such as RetinaNet.py:47-66's lr_schedule - which must return a float; it therefore
    replaces whatever ReduceLROnPlateau set at the end of the epoch before.  on_epoch_end writes logs['lr'].
    (fit_generator's older hook for any object with a `.schedule` attribute leaves instances of this class alone, so the schedule
    is applied once per epoch.)"""

    def __init__(self, schedule, verbose=0):
        super(LearningRateScheduler, self).__init__()
        self.schedule, self.verbose = schedule, verbose

    def on_epoch_begin(self, epoch, logs=None):
        lr = float(self.model.optimizer.lr)
        try:
            lr = self.schedule(epoch, lr)
        except TypeError:                                    # the old API: schedule(epoch)
            lr = self.schedule(epoch)
        if not isinstance(lr, (float, np.float32, np.float64)):
            raise ValueError('The output of the "schedule" function should be float.')
        self.model.optimizer.lr = float(lr)
        if self.verbose > 0:
            print('\nEpoch %05d: LearningRateScheduler setting learning rate to %s.' % (epoch + 1, lr))

    def on_epoch_end(self, epoch, logs=None):
        if logs is not None:
            logs['lr'] = float(self.model.optimizer.lr)


class CSVLogger(Callback):
    """keras.callbacks.CSVLogger(filename, separator=',', append=False).

    The file is opened in on_train_begin ('a' with append=True, and then the header is written only if the file is missing or
    empty; else 'w').  The columns are 'epoch' (0-based) plus the SORTED keys of the first epoch's logs; later epochs write those
    keys only, and a key missing once training was stopped is written as 'NA'.  Sequences are written as "[a, b]".  One row per
    epoch, flushed at once; on_train_end closes the file."""

    def __init__(self, filename, separator=',', append=False):
        super(CSVLogger, self).__init__()
        self.filename, self.sep, self.append = filename, separator, append
        self.writer = None
        self.keys = None
        self.append_header = True
        self.csv_file = None

    def on_train_begin(self, logs=None):
        if self.append:
            if os.path.exists(self.filename):
                with open(self.filename, 'r', newline='') as f:
                    self.append_header = not bool(len(f.readline()))
            mode = 'a'
        else:
            mode = 'w'
        self.csv_file = open(self.filename, mode, newline='')

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}

        def handle_value(k):
            if isinstance(k, str):
                return k
            if isinstance(k, np.ndarray) and k.ndim == 0:
                return k.item()
            if isinstance(k, (list, tuple, np.ndarray)):
                return '"[%s]"' % (', '.join(map(str, k)))
            return k
        if self.keys is None:
            self.keys = sorted(logs.keys())
        if getattr(self.model, 'stop_training', False):
            logs = dict((k, logs[k] if k in logs else 'NA') for k in self.keys)
        if not self.writer:
            class CustomDialect(csv.excel):
                delimiter = self.sep
            self.writer = csv.DictWriter(self.csv_file, fieldnames=['epoch'] + self.keys, dialect=CustomDialect)
            if self.append_header:
                self.writer.writeheader()
        row = OrderedDict({'epoch': epoch})
        row.update((key, handle_value(logs[key])) for key in self.keys)
        self.writer.writerow(row)
        self.csv_file.flush()

    def on_train_end(self, logs=None):
        if self.csv_file is not None:
            self.csv_file.close()
            self.csv_file = None
        self.writer = None
