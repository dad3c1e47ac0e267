#pragma once
#include <iostream>
#include <fstream>
#include <sstream>
