// refcv: the whole stand-in lives in opencv2/core/core.hpp (see the comment at its head).
#pragma once
#include "core/core.hpp"
