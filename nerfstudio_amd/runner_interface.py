"""What the training drivers ask of the runner they drive, stated once. Imports nothing of torch.cuda or the native library:
the CPU stand-ins of the tests derive from the same classes as the kernel schedules."""
from __future__ import annotations


class TrainStepRunner:
    """The runner of trainer.HipTrainer, dp_schedule.PipelinedExchange's segments and pipeline.TrainEngine
    (train_step.NerfactoTrainStep, which is forward_step.NerfactoForward plus this interface; tests: cpu_runner.CpuRunner, a
    toy schedule).

    Every runner provides
      n, origins, directions, camera_indices, target     the static batch buffers (`raw_origins`, `raw_directions` as well when
                                                          `cam_opt` is set: the kernels read the pose-corrected copies)
      anneal_dev                                          assigned by the trainer: the anneal exponent in device memory
      set_batch(origins, directions, camera_indices, target)
      written_params()                                    parameters whose gradient the backward writes (no zero-fill)
      apply_camera_corrections()
      forward_proposals(draw_jitter, need_enc=..., after_bins=...)
      forward_main_and_losses(updated, terms_ready=...)
      backward_all(updated)
      loss_dict(), outputs(), dist_per_ray
    and, for the uses named:
      backward_main(), backward_proposals()               the data-parallel segments
      backward_fork(updated), backward_join(updated)      the same with `side_stream` (the proposal chains beside the exchange)
      backward_cameras(updated, force=True), camera_reg   `cam_opt` set
      ray_terms_launch(select=...)                        `ray_terms_on` (select: the `pending_select` still to be consumed)
      loss_vals                                           `want_loss_vals`

    The attributes below are the optional capabilities the drivers read; a runner that does not state one has the default.
    Nearly every default selects a slower path with the same bits, which no test of bits notices: the drivers read the
    attributes plainly, tests/test_host_logic.py forbids probing them with getattr / hasattr, and
    tests/test_gpu_trainer_launch_counts.py counts the launches."""

    side_stream = None        # a stream for the proposal backward chains beside the main chain
    cam_opt = None            # the camera optimiser whose pose corrections the runner applies
    cameras_outside = False   # set by the trainer: the camera parts run around the iteration body, not inside it
    single_jitter = False     # one draw per level and ray in `jitter` (with it: the step prologue draws them)
    jitter = None
    bg_rays = None            # per-ray random background, drawn with the jitter
    prop_gates = None         # the proposal levels' gradient flags
    gates_precleared = False  # set by the trainer: it clears `prop_gates` with the gradients
    ray_terms_on = False      # the main field's per-ray terms are a launch of their own (`ray_terms_launch`)
    fuse_select = False       # `forward_proposals` selects the batch handed over in `pending_select`
    pending_select = None
    want_loss_vals = False    # set by TrainEngine: `losses` also leaves the loss values in `loss_vals`
    _loss_vals_fresh = False  # `loss_vals` holds the last iteration's values
    grad_lookup = None        # set by the trainer: {id(parameter): the arena's gradient view}


class PackedStepRunner:
    """The runner of ngp_trainer.NgpTrainer behind pipeline.NgpEngine (ngp_step.NgpTrainStep; tests: cpu_runner.CpuNgpRunner):
    set_batch, forward, loss, backward, outputs, `num_kept`, `target`."""

    # True: the backward writes through `grad_lookup` (the arena's gradient views, assigned by the engine); False: into
    # `param.grad`, which the engine then binds to those views for the duration of an iteration
    writes_arena_grads = False
    grad_lookup = None
