"""The denoiser's quality at its defaults, measured as profiles/denoise_quality.txt records it (tests/denoise_quality.py): relative MSE of the
8-SPP image and of its denoised version against the oracle's 2048-SPP image (tests/golden/denoise/), on the CPU through the host model. The
ratio rho = err(denoised) / err(noisy) must stay below (1 + rho_measured) / 2: half-way between the recorded value and "no better than not
denoising", because the ratio moves with the seed."""
import pytest

import denoise_quality as dq

RHO_MEASURED = {"room_textured": 0.0055, "room_manylights": 0.0070}  # profiles/denoise_quality.txt, the row of the defaults


@pytest.mark.parametrize("name", dq.SCENES)
def test_denoised_image_is_closer_to_the_converged_one(name):
    rho, e_noisy, e_den = dq.ratio(dq.state(name), dq.reference(name))
    print(f"{name}: relMSE noisy {e_noisy:.5f} denoised {e_den:.5f} rho {rho:.4f} (recorded {RHO_MEASURED[name]})")
    assert rho <= (1 + RHO_MEASURED[name]) / 2
