"""The training CLI with every label-free evaluation report switched on: each evaluation prints the report lines once, in the order
of the table (split_vae_amd/reports.py), behind the loss block -- for each of the three training loops."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CLI = ["--synthetic", "-no_label", "--batch_size", "8", "--training_steps", "1", "--log_every", "1", "--dtype", "f32"]      # 32 test images
FIRST_N = ["--latent_info", "32", "--recon_quality", "32", "--latent_dims", "32"]
LABEL_FREE = ["Test latent information (32 images, log N = 3.4657): z_g ", "Test reconstruction quality (32 images): PSNR ",
              "Test latent dimensions (32 images, log N = 3.4657): z_g active "]
# model flags, the report flags it accepts, the line of its bound, the start of the last line of its loss block
MODELS = {
    "lgvae": (["--model", "lgvae"], ["--iw_samples", "2"], "Test IW-2 bound: joint ", "            Total KL train loss: "),
    "lggmvae": (["--model", "lggmvae"], ["--gm_iw_samples", "2"], "Test IW-2 mixture bound: joint ", "            Test X Recon Loss: "),
    "gmvae": (["--model", "gmvae", "--y_size", "10"], ["--gm_iw_samples", "2"], "Test IW-2 mixture bound: joint ", "            Y KL train loss: "),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_every_evaluation_prints_the_report_lines_once_in_table_order(lib_built, tmp_path, monkeypatch, capsys, name):
    assert torch.cuda.is_available()
    from split_vae_amd import main as svmain
    model, bound, bound_line, loss_end = MODELS[name]
    monkeypatch.chdir(tmp_path)
    svmain.main(CLI + model + bound + FIRST_N)
    out = capsys.readouterr().out
    assert "Training done!" in out and "clipped" not in out and "Note: --knn_probe" not in out
    evaluations = out.split("Training step ")[1:]
    assert len(evaluations) == 2                                                  # steps 0 and 1
    want = [bound_line] + LABEL_FREE
    for text in evaluations:
        lines = text.split("Training time:")[0].split("Training done!")[0].splitlines()
        reports = [i for i, l in enumerate(lines) if l.startswith("Test ")]      # the loss block's lines are indented
        assert len(reports) == len(want) and all(lines[i].startswith(w) for i, w in zip(reports, want)), text
        assert reports == list(range(reports[0], reports[0] + len(want)))        # nothing printed between them
        loss = [i for i, l in enumerate(lines) if l.startswith(loss_end)]
        assert loss and reports[0] > loss[-1], text
